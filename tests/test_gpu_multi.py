"""GPU tests of frames on several devices that carry a covariance or are sampled adaptively (include/ptr_multi.h, csrc/kernels/multi.hip,
csrc/host/multi.cpp).  The reference is always the single-device result: the numpy restatement tests/adaptive_ref.py for the protocol on
synthetic samples, DeviceScene.render_adaptive / render_image_cov for frames of the scene.  Everything is compared bit for bit.

A device id may repeat in an id list, so one GPU runs every partition, the exchange between them and the gather; an id -(id + 1) sends that
partition's bands through the pinned-host staging path.  The scene is tests/golden/cornell_small_mesh.scene at depth 4, seed 1337."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import adaptive_ref
import multi_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(ROOT, "scenes")

W, H, MIN, STEP, MAX = 88, 72, 4, 4, 16          # 9 bands
ID_LISTS = [[0], [0, 0], [0, 0, 0], [0] * 9, [0, -1, -1]]
list_id = lambda ids: "ids" + "_".join(str(i) for i in ids)


# --------------------------------------------------------------------------- 1. the protocol is the restatement
PROBE_CASES = [(1, 1, [0]), (5, 3, [0]), (67, 45, [0]), (67, 45, [0, 0]), (67, 45, [0, 0, 0]), (67, 45, [0] * 6), (67, 45, [0, -1, -1]),
               (130, 70, [0, 0]), (130, 70, [0] * 9),
               # a list longer than the image has bands: the partitions past the last band own no pixel and still meet at every barrier
               (5, 3, [0, 0]), (67, 45, [0] * 7)]
_synthetic = {}


def synthetic(w, h):
    """Samples, parameters and the single-device restatement of a size, computed once."""
    if (w, h) not in _synthetic:
        max_spp = 16 if w == 130 else 12
        x = adaptive_ref.synthetic_samples(max_spp, h, w)
        thr = multi_ref.median_threshold(x, MIN, STEP)
        _synthetic[(w, h)] = (x, thr, max_spp, adaptive_ref.adaptive_ref(x, adaptive_ref.params(MIN, max_spp, STEP, thr)))
    return _synthetic[(w, h)]


@pytest.mark.parametrize("w,h,ids", PROBE_CASES, ids=lambda v: list_id(v) if isinstance(v, list) else str(v))
def test_protocol_is_the_restatement(w, h, ids):
    """The partition loop of the renderer - update, pack, exchange, unpack, select, compact, finish, gather - fed from synthetic samples.
    tests/test_multi_host.py shows that on the 67x45 and 130x70 inputs a missing or a stale halo changes at least 20 final counts."""
    x, thr, max_spp, want = synthetic(w, h)
    rgb, cov, count, info = pt.multi_adaptive_debug_frame(x, pt.PtrAdaptiveParams(MIN, max_spp, STEP, thr), ids)
    assert count.dtype == np.uint32 and np.array_equal(count, want.count)
    assert np.array_equal(rgb, want.rgb, equal_nan=True) and np.array_equal(cov, want.cov, equal_nan=True)
    assert info.rounds == want.rounds and info.active_counts() == want.active_after
    assert info.totalSamples == int(want.count.sum()) and info.pixelsAtMax == int((want.count == max_spp).sum())
    if w >= 67:
        assert len(np.unique(want.count)) >= 3           # a mixed frame: some pixels stop at every round


# --------------------------------------------------------------------------- 2. the frame is the single-device frame
@pytest.fixture(scope="module")
def cornell():
    host = pt.HostScene.load(os.path.join(GOLDEN, "cornell_small_mesh.scene"), SCENES)
    return host, pt.DeviceScene(host.desc, 0, keepalive=host)


@pytest.fixture(scope="module")
def frame(cornell):
    """The 88x72 frame the tests below share: the samples of a uniform 16-spp frame, the restatement on them with the threshold at the
    median of its own dilated first-round error, and the adaptive frame of one device."""
    host, dev = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    samples = dev.debug_samples(s, MAX)
    thr = multi_ref.median_threshold(samples, MIN, STEP)
    want = adaptive_ref.adaptive_ref(samples, adaptive_ref.params(MIN, MAX, STEP, thr))
    p = pt.PtrAdaptiveParams(MIN, MAX, STEP, thr)
    single = dev.render_adaptive(s, p)
    return s, p, samples, want, single


def same_frame(out, single, what):
    rgb, cov, count, _, info = single
    assert np.array_equal(out["rgb"], rgb) and np.array_equal(out["cov"], cov) and np.array_equal(out["count"], count), what
    got = out["info"]
    assert got.rounds == info.rounds and got.active_counts() == info.active_counts(), what
    assert got.totalSamples == info.totalSamples and got.pixelsAtMax == info.pixelsAtMax, what


def test_the_input_splits_the_image(frame):
    """Conditions on the input, from the restatement alone: 20 % to 80 % of the pixels end at minSpp and at least three distinct counts
    occur.  Printed, not asserted: how many final counts a missing or a stale halo would change on this frame's own samples (the
    discriminating input is test 1's)."""
    _, p, samples, want, single = frame
    assert np.array_equal(single[2], want.count)          # the single-device frame is the restatement of its own samples
    at_min = float((want.count == MIN).mean())
    print("pixels that end at %d spp: %.1f %%; counts %s" % (MIN, 100.0 * at_min, np.unique(want.count, return_counts=True)))
    ref_p = adaptive_ref.params(MIN, MAX, STEP, p.threshold)
    for halo in ("none", "stale"):
        changed = int((multi_ref.multi_ref(samples, ref_p, 3, halo=halo).count != want.count).sum())
        print("3 partitions, halo %s: %d of %d final counts would change" % (halo, changed, W * H))
    assert 0.2 <= at_min <= 0.8 and len(np.unique(want.count)) >= 3


@pytest.mark.parametrize("ids", ID_LISTS, ids=list_id)
def test_frame_is_the_single_device_frame(cornell, frame, ids):
    host, _ = cornell
    s, p, _, _, single = frame
    out = pt.render_multi_adaptive(host.desc, s, p, device_ids=ids)
    same_frame(out, single, ids)
    multi, count = out["multi"], single[2]
    assert multi.parts == len(ids) and multi.stagedParts == sum(1 for i in ids if i < 0)
    per_part = multi.per_part()
    assert sum(v[0] for v in per_part) == out["info"].totalSamples == out["stats"].samples == int(count.sum())
    band_of_row = np.arange(H) // pt.BAND_ROWS
    for q, (samples_q, render_q, wait_q) in enumerate(per_part):
        assert samples_q == int(count[band_of_row % len(ids) == q].sum()), q
        assert render_q > 0 and 0 <= wait_q <= render_q
    assert out["stats"].totalSeconds > 0 and out["stats"].traceLaunches > 0


def test_device_counts(cornell, frame):
    host, _ = cornell
    s, p, _, _, single = frame
    same_frame(pt.render_multi_adaptive(host.desc, s, p, n_devices=1), single, "n_devices=1")
    with pytest.raises(pt.PtrError, match="ptr_render_multi_adaptive: .*devices requested"):
        pt.render_multi_adaptive(host.desc, s, p, n_devices=pt.device_count() + 1)
    with pytest.raises(pt.PtrError, match="ptr_render_multi_cov: .*devices requested"):
        pt.render_multi_cov(host.desc, s, 6, n_devices=pt.device_count() + 1)
    with pytest.raises(pt.PtrError, match="ptr_multi_debug_adaptive_on: no such HIP device"):
        pt.render_multi_adaptive(host.desc, s, p, device_ids=[0, pt.device_count()])
    with pytest.raises(pt.PtrError, match="ptr_multi_debug_adaptive_frame: no such HIP device"):
        pt.multi_adaptive_debug_frame(np.ones((MAX, 8, 8, 3), np.float32), p, [-pt.device_count() - 1])


# --------------------------------------------------------------------------- 3. sub-passes
def test_sub_passes_change_nothing(cornell, frame):
    """PTR_MAX_ITEMS=1024: every partition's rounds arrive in sub-passes, split by its own list length."""
    host, _ = cornell
    s, p, _, _, single = frame
    os.environ["PTR_MAX_ITEMS"] = "1024"
    try:
        out = pt.render_multi_adaptive(host.desc, s, p, device_ids=[0, 0, 0])
    finally:
        del os.environ["PTR_MAX_ITEMS"]
    same_frame(out, single, "PTR_MAX_ITEMS=1024")


# --------------------------------------------------------------------------- 4. uniform covariance
@pytest.fixture(scope="module")
def uniform(cornell):
    host, dev = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    rgb, cov, _ = dev.render_image_cov(s, 6)
    plain, _ = pt.render_multi(host.desc, s, 6, device_ids=[0, 0])
    return s, rgb, cov, plain


@pytest.mark.parametrize("ids", ID_LISTS, ids=list_id)
def test_uniform_covariance(cornell, uniform, ids):
    host, _ = cornell
    s, rgb, cov, plain = uniform
    out = pt.render_multi_cov(host.desc, s, 6, device_ids=ids)
    assert np.array_equal(out["rgb"], rgb) and np.array_equal(out["cov"], cov)
    assert np.array_equal(out["rgb"], plain)
    assert out["multi"].parts == len(ids) and out["multi"].stagedParts == sum(1 for i in ids if i < 0)
    assert sum(v[0] for v in out["multi"].per_part()) == out["stats"].samples == 6 * W * H
    assert out["albedo"] is None and out["normal"] is None


# --------------------------------------------------------------------------- 5. AOVs and the denoiser
def test_aovs_and_the_denoiser(cornell, frame, uniform):
    host, dev = cornell
    s, p, _, _, single = frame
    albedo, normal = dev.render_aovs(s, 0)
    out = pt.render_multi_adaptive(host.desc, s, p, device_ids=[0, 0, 0], want_aovs=True)
    same_frame(out, single, "with AOVs")
    assert np.array_equal(out["albedo"], albedo) and np.array_equal(out["normal"], normal)
    want = pt.denoise(single[0], albedo, normal, cov=single[1])
    assert np.array_equal(pt.denoise(out["rgb"], out["albedo"], out["normal"], cov=out["cov"]), want)
    assert np.isfinite(want).all() and not np.array_equal(want, single[0])
    _, rgb, cov, _ = uniform
    flat = pt.render_multi_cov(host.desc, s, 6, device_ids=[0, 0], want_aovs=True)
    assert np.array_equal(flat["albedo"], albedo) and np.array_equal(flat["normal"], normal)
    assert np.array_equal(pt.denoise(flat["rgb"], flat["albedo"], flat["normal"], cov=flat["cov"]), pt.denoise(rgb, albedo, normal, cov=cov))
    # cov and count are optional
    bare = pt.render_multi_adaptive(host.desc, s, p, device_ids=[0, 0], want_cov=False, want_count=False)
    assert np.array_equal(bare["rgb"], single[0]) and bare["cov"] is None and bare["count"] is None


# --------------------------------------------------------------------------- 6. nothing cached was disturbed
def test_plain_multi_frame_before_and_after(cornell, frame):
    host, dev = cornell
    s, p, _, _, single = frame
    before, _ = pt.render_multi(host.desc, s, 5, device_ids=[0, 0, 0])
    same_frame(pt.render_multi_adaptive(host.desc, s, p, device_ids=[0, 0, 0]), single, "between two plain frames")
    after, _ = pt.render_multi(host.desc, s, 5, device_ids=[0, 0, 0])
    assert np.array_equal(before, after) and np.array_equal(dev.render_image(s, 5)[0], before)


# --------------------------------------------------------------------------- 7. the plain frame goes through the same driver
def test_plain_frame_with_empty_partitions(cornell):
    """37x21: three bands, the last of five rows, ragged 8x8 blocks.  The fourth partition owns no band and must not disturb the frame."""
    host, dev = cornell
    s = host.settings_for(width=37, height=21, max_depth=4, seed=1337)
    want = dev.render_image(s, 5)[0]
    for ids in ([0] * 4, [0, -1, 0, 0]):
        got, stats = pt.render_multi(host.desc, s, 5, device_ids=ids)
        assert np.array_equal(got, want), ids
        assert stats.samples == 37 * 21 * 5, ids


def test_plain_frame_takes_the_sample_counts_a_covariance_refuses(cornell):
    """spp = 1, and spp = 0, which renders one sample and reports one."""
    host, dev = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    want = dev.render_image(s, 1)[0]
    for spp in (1, 0):
        got, stats = pt.render_multi(host.desc, s, spp, device_ids=[0, 0, 0])
        assert np.array_equal(got, want), spp
        assert stats.samples == W * H and stats.avgMsPerSample > 0, spp


def test_plain_frame_in_sub_passes(cornell):
    """PTR_MAX_ITEMS=1024: every partition renders its six samples in six passes, whose stats add up in the frame's."""
    host, dev = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    want = dev.render_image(s, 6)[0]
    os.environ["PTR_MAX_ITEMS"] = "1024"
    try:
        got, stats = pt.render_multi(host.desc, s, 6, device_ids=[0, 0, 0])
    finally:
        del os.environ["PTR_MAX_ITEMS"]
    assert np.array_equal(got, want)
    assert stats.samples == W * H * 6


# The child of test_plain_frame_verbose_report: argv = root.
PLAIN_VERBOSE_CHILD = """
import importlib, os, sys
root = sys.argv[1]
sys.path.insert(0, root)
pt = importlib.import_module("metal-pathtracer-arm64_amd")
host = pt.HostScene.load(os.path.join(root, "tests", "golden", "cornell_small_mesh.scene"), os.path.join(root, "scenes"))
s = host.settings_for(width=%d, height=%d, max_depth=4, seed=1337)
pt.render_multi(host.desc, s, 4, n_devices=1, verbose=True)
""" % (W, H)


def test_plain_frame_verbose_report():
    """The plain frame reports two kinds of line: the call's, and one per partition with its bands and render time."""
    r = subprocess.run([sys.executable, "-c", PLAIN_VERBOSE_CHILD, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("[ptr]")]
    assert len(lines) == 2, lines
    assert re.match(r"\[ptr\] 1 device\(s\): scene preparation [0-9.]+ s, slowest upload [0-9.]+ s, slowest render \+ hand-over [0-9.]+ s, "
                    r"whole call [0-9.]+ s$", lines[0]), lines[0]
    assert re.match(r"\[ptr\]   device 0: 9 bands, render [0-9.]+ s$", lines[1]), lines[1]


def test_plain_frame_refusals_that_need_a_device(cornell):
    host, _ = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    with pytest.raises(pt.PtrError, match="ptr_render_multi: .*devices requested"):
        pt.render_multi(host.desc, s, 4, n_devices=pt.device_count() + 1)
    with pytest.raises(pt.PtrError, match="ptr_debug_render_multi_on: no such HIP device"):
        pt.render_multi(host.desc, s, 4, device_ids=[0, pt.device_count()])
