"""The resumable frame of include/ptr_frame.h restated in numpy, written from that header's text and sharing no code with the product.

It stands on tests/adaptive_ref.py for what the header takes word for word from ptr_adaptive.h (Update and e: round_ref; E: dilate; the
first-list order; the zero state).  FrameRef(samples) holds samples[S][H][W][3], the per-sample values a uniform frame of S samples
would see; log gets one (n_min, |S|, |L| after) per round of a refine.
"""
from types import SimpleNamespace

import numpy as np

from adaptive_ref import dilate, pixel_order, round_ref, zero_state

F = np.float32
NO_SELECT = SimpleNamespace(maxSpp=0, threshold=F(0))   # round_ref's own select is not used here


class FrameRef:
    def __init__(self, samples):
        samples = np.asarray(samples, dtype=F)[..., :3]
        self.height, self.width = samples.shape[1:3]
        self.flat = samples.reshape(samples.shape[0], self.height * self.width, 3)
        self.order = pixel_order(self.width, self.height)
        self.state = zero_state(self.height * self.width)
        self.log = []

    def _update(self, entries, n_before, spp):
        """Update: the samples n_before .. n_before + spp - 1 of the listed pixels; e from the new count."""
        x = self.flat[n_before:n_before + spp][:, entries]
        self.state, _, _ = round_ref(self.width, self.height, NO_SELECT, n_before, x, entries, self.state)

    def _select(self, entries, p):
        """The entries that stay: n_p < maxSpp and E_p > threshold, E over the whole image."""
        big = dilate(self.state["e"], self.width, self.height)
        return entries[(self.state["n"][entries] < p.maxSpp) & (big[entries] > p.threshold)]

    def accumulate(self, spp):
        n = self.state["n"]
        assert spp >= 1 and (n == n[0]).all(), "accumulate needs a uniform frame"
        self._update(self.order, int(n[0]), spp)

    def refine(self, p):
        """Returns a namespace: rounds, active_after, total_samples, pixels_at_max."""
        out = SimpleNamespace(rounds=0, active_after=[], total_samples=0)
        n = self.state["n"]
        empty = bool((n == 0).all())
        if empty:
            self._update(self.order, 0, p.minSpp)
            out.total_samples += p.minSpp * self.order.size
        else:
            assert (n >= 2).all(), "refine needs two samples in every pixel"
        L = self._select(self.order, p)
        if empty:
            out.rounds, out.active_after = 1, [int(L.size)]
        while L.size:
            counts = self.state["n"][L]
            n_min = int(counts.min())
            in_s = counts == n_min
            S = L[in_s]
            k = min(p.stepSpp, p.maxSpp - n_min)
            self._update(S, n_min, k)
            stays = np.isin(S, self._select(S, p))
            keep = np.ones(L.size, bool)
            keep[in_s] = stays
            L = L[keep]
            out.rounds += 1
            out.active_after.append(int(L.size))
            out.total_samples += k * int(S.size)
            self.log.append((n_min, int(S.size), int(L.size)))
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
