"""The adaptive frame of include/ptr_adaptive.h restated in numpy, written from that header's text and sharing no code with the product.

Like stats_ref.welford32: float32 throughout, one numpy operation per line of the header - every numpy float32 operation rounds once
(IEEE), as the unfused device arithmetic does, so it reproduces the kernels' bits.

round_ref: one round (or one sub-pass of a round) on explicit state: update -> select -> compact.
adaptive_ref: the whole frame from samples[maxSpp][H][W][3], the per-sample values a uniform frame of maxSpp samples would see.
"""
from types import SimpleNamespace

import numpy as np

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # rr, gg, bb, rg, rb, gb
SYM = ((0, 3, 4), (3, 1, 5), (4, 5, 2))                    # the entry of M that holds C[c][d]
K = (np.float32(0.2126), np.float32(0.7152), np.float32(0.0722))
F = np.float32


def params(min_spp, max_spp, step_spp, threshold):
    return SimpleNamespace(minSpp=int(min_spp), maxSpp=int(max_spp), stepSpp=int(step_spp), threshold=F(threshold))


def pixel_order(width, height):
    """The first active list: 8-row bands top to bottom, each walked in 8x8 blocks left to right, each block row-major."""
    out = []
    for ty in range(0, height, 8):
        for tx in range(0, width, 8):
            for y in range(ty, min(ty + 8, height)):
                for x in range(tx, min(tx + 8, width)):
                    out.append(y * width + x)
    return np.array(out, dtype=np.uint32)


def zero_state(pixels):
    return {"sum": np.zeros((pixels, 3), F), "mean": np.zeros((pixels, 3), F), "m": np.zeros((pixels, 6), F),
            "n": np.zeros(pixels, np.uint32), "e": np.zeros(pixels, F)}


def pixel_error(mean, m, n):
    """e of the header for pixels with `n` samples each: mean [P, 3], m [P, 6] -> [P]."""
    with np.errstate(all="ignore"):
        cov = m / (F(n) * F(n - 1))
        v = np.zeros(mean.shape[0], F)
        for c in range(3):
            for d in range(3):
                v = v + (K[c] * K[d]) * cov[:, SYM[c][d]]
        v = np.where(np.isfinite(v) & (v > 0), v, F(0))
        l = (K[0] * mean[:, 0] + K[1] * mean[:, 1]) + K[2] * mean[:, 2]
        l = np.where(l > 0, l, F(0))
        return (np.sqrt(v) / (l + F(1e-2))).astype(F)


def dilate(e, width, height):
    """E of the header for every pixel of the image: e [H*W] -> [H*W]."""
    e2 = e.reshape(height, width)
    big = np.zeros((height, width), F)
    with np.errstate(invalid="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ys = slice(max(0, -dy), height - max(0, dy))
                xs = slice(max(0, -dx), width - max(0, dx))
                q = e2[max(0, dy):height - max(0, -dy), max(0, dx):width - max(0, -dx)]
                cur = big[ys, xs]
                big[ys, xs] = np.where(q > cur, q, cur)
    return big.reshape(-1)


def round_ref(width, height, p, n_before, samples, active, state, last=True):
    """samples [round_spp, len(active), >= 3] in list order; state as zero_state().  Returns (new state, next list, E [H*W] or None)."""
    x = np.asarray(samples, dtype=F)[..., :3]
    active = np.asarray(active, dtype=np.uint32)
    st = {k: v.copy() for k, v in state.items()}
    total, mean, m = st["sum"][active], st["mean"][active], st["m"][active]
    with np.errstate(all="ignore"):
        for c in range(x.shape[0]):
            k = n_before + c + 1
            total = total + x[c]
            d = x[c] - mean
            mean = mean + d / F(k)
            e = x[c] - mean
            for i, (a, b) in enumerate(PAIRS):
                m[:, i] = m[:, i] + d[:, a] * e[:, b]
    n = n_before + x.shape[0]
    st["sum"][active], st["mean"][active], st["m"][active] = total, mean, m
    st["n"][active] = n
    if not last:
        return st, active.copy(), None
    st["e"][active] = pixel_error(mean, m, n)
    big = dilate(st["e"], width, height)
    keep = (st["n"][active] < p.maxSpp) & (big[active] > p.threshold)
    return st, active[keep], big


def adaptive_ref(samples, p):
    """samples [maxSpp, H, W, 3].  Returns a namespace: rgb [H, W, 3], cov [H, W, 6], count [H, W] uint32, lists (the active list of every
    round, the first being pixel_order), active_after (the length of the list after every round), e and E (the error map and its dilation
    after every round, [H, W]), rounds."""
    samples = np.asarray(samples, dtype=F)
    height, width = samples.shape[1:3]
    flat = samples.reshape(samples.shape[0], height * width, 3)
    st = zero_state(height * width)
    active = pixel_order(width, height)
    out = SimpleNamespace(lists=[], active_after=[], e=[], E=[], rounds=0)
    n = 0
    while active.size > 0 and n < p.maxSpp:
        spp = p.minSpp if n == 0 else min(p.stepSpp, p.maxSpp - n)
        out.lists.append(active)
        st, active, big = round_ref(width, height, p, n, flat[n:n + spp][:, active], active, st)
        n += spp
        out.active_after.append(int(active.size))
        out.e.append(st["e"].reshape(height, width).copy())
        out.E.append(big.reshape(height, width).copy())
        out.rounds += 1
    with np.errstate(all="ignore"):
        count = st["n"]
        out.rgb = (st["sum"] / count.astype(F)[:, None]).reshape(height, width, 3)
        out.cov = (st["m"] / (count.astype(F) * (count - 1).astype(F))[:, None]).reshape(height, width, 6)
    out.count = count.reshape(height, width)
    return out


def synthetic_samples(spp, height, width, seed=7):
    """Per-sample values of the kind a path tracer makes (lognormal, a few 1e3 outliers), with exact zeros in the last two rows (a
    background) and one pixel whose samples are NaN."""
    rng = np.random.default_rng(seed)
    base = rng.lognormal(mean=-1.0, sigma=1.0, size=(spp, height, width, 1))
    x = np.abs(base * rng.uniform(0.2, 1.0, size=(1, height, width, 3)) * (1.0 + 0.2 * rng.standard_normal((spp, height, width, 3))))
    hot = rng.random((spp, height, width)) < 0.01
    x[hot] = x[hot] + 1.0e3
    if height > 2:
        x[:, -2:] = 0.0
    x = x.astype(F)
    if height * width > 4:
        x[:, height // 2, width // 2] = np.nan
    return x
