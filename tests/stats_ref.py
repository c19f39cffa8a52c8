"""The covariance of include/ptr_stats.h restated in numpy, written from that header's text and sharing no code with the product.

welford32: the header's recurrence in float32, vectorised over the pixels, one numpy operation per line of the header - every numpy
float32 operation rounds once (IEEE), as the unfused device arithmetic does, so it reproduces the kernel's bits.
two_pass64: the same quantity the textbook way in float64 (mean first, then the centred products): the yardstick for what float32 and
the streaming form cost.
Both take samples [n, ..., 3] in sample order and return [..., 6] in the order rr, gg, bb, rg, rb, gb.
"""
import numpy as np

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # rr, gg, bb, rg, rb, gb


def welford32(samples):
    x = np.asarray(samples, dtype=np.float32)
    n = x.shape[0]
    mean = np.zeros(x.shape[1:], np.float32)
    m = np.zeros(x.shape[1:-1] + (6,), np.float32)
    with np.errstate(all="ignore"):
        for k in range(1, n + 1):
            d = x[k - 1] - mean
            mean = mean + d / np.float32(k)
            e = x[k - 1] - mean
            for i, (a, b) in enumerate(PAIRS):
                m[..., i] = m[..., i] + d[..., a] * e[..., b]
        return m / (np.float32(n) * np.float32(n - 1))


def two_pass64(samples):
    x = np.asarray(samples, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    c = x - x.mean(axis=0)
    out = np.empty(x.shape[1:-1] + (6,), np.float64)
    for i, (a, b) in enumerate(PAIRS):
        out[..., i] = (c[..., a] * c[..., b]).sum(axis=0) / (n * (n - 1.0))
    return out


def relative_error(w32, c64):
    """max over pixels and entries ab of |w32 - c64| / sqrt(C_aa C_bb) (pixels with a zero C_aa C_bb are left out: the caller checks
    those for exact zeros)."""
    w32 = np.asarray(w32, np.float64)
    scale = np.stack([np.sqrt(c64[..., a] * c64[..., b]) for a, b in PAIRS], axis=-1)
    ok = scale > 0
    return float((np.abs(w32 - c64)[ok] / scale[ok]).max()) if ok.any() else 0.0


def heavy_tailed_samples(n, pixels=4096, seed=2024):
    """Synthetic per-sample accumulators [n, pixels, 3] of the kind a path tracer makes: lognormal (sigma 1.5) radiance with correlated
    channels, a few 1e4 outliers (fireflies), and - the last 64 pixels - samples that are all equal (a converged or black pixel)."""
    rng = np.random.default_rng(seed + n)
    base = rng.lognormal(mean=-1.0, sigma=1.5, size=(n, pixels, 1))
    tint = rng.uniform(0.2, 1.0, size=(1, pixels, 3)) * (1.0 + 0.2 * rng.standard_normal((n, pixels, 3)))
    x = np.abs(base * tint)
    hot = rng.random((n, pixels)) < 0.01
    x[hot] = x[hot] + 1.0e4 * rng.uniform(0.5, 1.0, size=(int(hot.sum()), 3))
    x[:, -64:, :] = rng.uniform(0.0, 2.0, size=(1, 64, 3))
    x[:, -8:, :] = 0.0
    return x.astype(np.float32)


# The largest relative_error(welford32, two_pass64) over heavy_tailed_samples(n), n in {2, 3, 7, 64}, measured on the CPU: 1.281e-4, at
# n = 2 (a 1e4 outlier beside a sample near 0.1: the difference of the two keeps seven digits of the larger one).  The bound the tests
# assert is four times that, to cover other inputs; tests/test_stats_host.py measures it again and holds it against the bound.
MEASURED_WORST = 1.281e-4
BOUND = 4.0 * MEASURED_WORST
