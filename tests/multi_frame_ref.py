"""The resumable frame on several devices of include/ptr_multi_frame.h restated in numpy, written from that header's text and sharing no
code with the product.  It stands on tests/adaptive_ref.py for what the header takes from ptr_adaptive.h (Update and e: round_ref; E:
dilate; the zero state): P partitions of 8-row bands, each with image-order state arrays of its own whose e knows the other partitions'
rows only through the halo - publish into `published`, collect from it.

MultiFrameRef(samples, parts, halo):
  halo = "true"                         the protocol of the header;
  halo = "none"                         nothing is exchanged: rows of other partitions count as e = 0;
  halo = "stale_start"                  no collect before the start-list Select of a refine;
  halo = "no_publish_after_accumulate"  Accumulate (a refine's first one included) does not publish.
The three wrong variants exist to show that an input discriminates (tests/test_multi_frame_host.py).

log gets one (n_min, sum of |S_p|, sum of |L_p| after) per round of a refine, as FrameRef's does; parts_log one list per round of
(|S_p|, |L_p| before the round) per partition."""
from types import SimpleNamespace

import numpy as np

from adaptive_ref import dilate, round_ref, synthetic_samples, zero_state

BAND = 8
F = np.float32
NO_SELECT = SimpleNamespace(maxSpp=0, threshold=F(0))   # round_ref's own select is not used here
HALOS = ("true", "none", "stale_start", "no_publish_after_accumulate")


def first_list(width, height, part, parts):
    """Partition `part`'s own pixels: its bands top to bottom, each walked in 8x8 blocks left to right, each block row-major."""
    out = []
    for b in range(part, (height + BAND - 1) // BAND, parts):
        for tx in range(0, width, 8):
            for y in range(b * BAND, min(b * BAND + BAND, height)):
                for x in range(tx, min(tx + 8, width)):
                    out.append(y * width + x)
    return np.array(out, dtype=np.uint32)


def quiet_band_samples(spp, height, width):
    """synthetic_samples with image rows 7 .. 16 - band 1 and the row on either side of it - made constant (no error at all), except
    six pixels in the middle of band 1 whose first sample is a spike and whose other samples are zero: their error stays near 1
    whatever their count.  A first refine takes them and their neighbours to maxSpp while the other bands stop at every count, so in a
    second refine the partition that owns band 1 alone starts with a list of pixels at the old maxSpp only and has an empty S_p until
    the others have caught up."""
    assert height > 17 and width > 33
    x = synthetic_samples(spp, height, width).copy()
    x[:, 7:17] = F(0.25)
    x[:, 11:13, 30:33] = F(0)
    x[0, 11:13, 30:33] = F(1000)
    return x


class MultiFrameRef:
    def __init__(self, samples, parts, halo="true"):
        assert halo in HALOS and parts >= 1
        samples = np.asarray(samples, dtype=F)[..., :3]
        self.height, self.width = samples.shape[1:3]
        self.pixels = self.height * self.width
        self.flat = samples.reshape(samples.shape[0], self.pixels, 3)
        self.parts, self.halo = parts, halo
        self.bands = (self.height + BAND - 1) // BAND
        self.orders = [first_list(self.width, self.height, q, parts) for q in range(parts)]
        self.owner = (np.arange(self.pixels) // self.width // BAND) % parts
        self.states = [zero_state(self.pixels) for _ in range(parts)]
        self.published = np.zeros((self.height, self.width), F)      # by image row: what the row's owner published last
        self.log, self.parts_log = [], []

    # ---- the halo
    def _own_bands(self, q):
        return range(q, self.bands, self.parts)

    def _publish(self, q):
        if self.parts == 1 or self.halo == "none":
            return
        e2 = self.states[q]["e"].reshape(self.height, self.width)
        for b in self._own_bands(q):
            last = min(b * BAND + BAND, self.height) - 1
            self.published[b * BAND] = e2[b * BAND]
            self.published[last] = e2[last]

    def _collect(self, q):
        if self.parts == 1 or self.halo == "none":
            return
        e2 = self.states[q]["e"].reshape(self.height, self.width)
        for b in self._own_bands(q):
            if b > 0:
                e2[b * BAND - 1] = self.published[b * BAND - 1]
            if b * BAND + BAND < self.height:
                e2[b * BAND + BAND] = self.published[b * BAND + BAND]

    # ---- Update and Select of one partition
    def _update(self, q, entries, n_before, spp):
        x = self.flat[n_before:n_before + spp][:, entries]
        self.states[q], _, _ = round_ref(self.width, self.height, NO_SELECT, n_before, x, entries, self.states[q])

    def _select(self, q, entries, p):
        st = self.states[q]
        big = dilate(st["e"], self.width, self.height)
        return entries[(st["n"][entries] < p.maxSpp) & (big[entries] > p.threshold)]

    # ---- the state, each pixel from its owner
    @property
    def state(self):
        out = zero_state(self.pixels)
        for q in range(self.parts):
            mine = self.owner == q
            for k in out:
                out[k][mine] = self.states[q][k][mine]
        return out

    export_state = state.fget

    def import_state(self, state):
        for q in range(self.parts):
            mine = self.owner == q
            for k in self.states[q]:
                self.states[q][k][mine] = state[k][mine]
        for q in range(self.parts):
            self._publish(q)

    def reset(self):
        self.states = [zero_state(self.pixels) for _ in range(self.parts)]
        self.published[:] = 0

    # ---- the calls
    def _accumulate_all(self, n, spp):
        for q in range(self.parts):
            if self.orders[q].size:
                self._update(q, self.orders[q], n, spp)
                if self.halo != "no_publish_after_accumulate":
                    self._publish(q)

    def accumulate(self, spp):
        n = self.state["n"]
        assert spp >= 1 and (n == n[0]).all(), "accumulate needs a uniform frame"
        self._accumulate_all(int(n[0]), spp)

    def refine(self, p):
        """Returns a namespace: rounds, active_after, total_samples, pixels_at_max."""
        out = SimpleNamespace(rounds=0, active_after=[], total_samples=0)
        n = self.state["n"]
        empty = bool((n == 0).all())
        if empty:
            self._accumulate_all(0, p.minSpp)
            out.total_samples += p.minSpp * self.pixels
        else:
            assert (n >= 2).all(), "refine needs two samples in every pixel"
        # (all partitions meet) collect, the start lists
        lists = []
        for q in range(self.parts):
            if self.halo != "stale_start":
                self._collect(q)
            lists.append(self._select(q, self.orders[q], p))
        total = sum(int(L.size) for L in lists)
        if empty:
            out.rounds, out.active_after = 1, [total]
        while total:
            n_min = min(int(self.states[q]["n"][L].min()) for q, L in enumerate(lists) if L.size)
            k = min(p.stepSpp, p.maxSpp - n_min)
            in_s = [self.states[q]["n"][L] == n_min for q, L in enumerate(lists)]
            self.parts_log.append([(int(s.sum()), int(L.size)) for s, L in zip(in_s, lists)])
            for q, L in enumerate(lists):                             # update over S_p, publish
                if in_s[q].any():
                    self._update(q, L[in_s[q]], n_min, k)
                    self._publish(q)
            for q, L in enumerate(lists):                             # (all partitions meet) collect, select on S_p, merge
                if not in_s[q].any():
                    continue
                self._collect(q)
                S = L[in_s[q]]
                keep = np.ones(L.size, bool)
                keep[in_s[q]] = np.isin(S, self._select(q, S, p))
                lists[q] = L[keep]
            total = sum(int(L.size) for L in lists)
            moved = sum(int(s.sum()) for s in in_s)
            out.rounds += 1
            out.active_after.append(total)
            out.total_samples += k * moved
            self.log.append((n_min, moved, total))
        out.pixels_at_max = int((self.state["n"] == p.maxSpp).sum())
        return out

    def resolve(self):
        """(rgb [H, W, 3], cov [H, W, 6], count [H, W] uint32)"""
        st, shape = self.state, (self.height, self.width)
        with np.errstate(all="ignore"):
            count = st["n"]
            rgb = st["sum"] / count.astype(F)[:, None]
            cov = st["m"] / (count.astype(F) * (count - np.uint32(1)).astype(F))[:, None]
        return rgb.reshape(shape + (3,)), cov.reshape(shape + (6,)), count.reshape(shape).copy()
