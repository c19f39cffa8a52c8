"""GPU tests of adaptive sampling (include/ptr_adaptive.h, csrc/kernels/adaptive.hip, csrc/host/adaptive.cpp): the round kernels against
the numpy restatement (tests/adaptive_ref.py) through the test-only probe, the frame against the restatement of its own samples, every
pixel against the uniform frame of its count, the invariances, the limits, and the frame under the denoiser and the CLI.

Unless stated the scene is tests/golden/cornell_small_mesh.scene at depth 4, seed 1337.  Everything is compared bit for bit: nothing
here asserts that an adaptive frame is better than a uniform one (that is measured by tools/adaptive_cost.py)."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import adaptive_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(ROOT, "scenes")
STATE_KEYS = ("sum", "mean", "m", "n", "e")
UNWRITTEN = 0xFFFFFFFF


def open_scene(name="cornell_small_mesh.scene"):
    host = pt.HostScene.load(os.path.join(GOLDEN, name), SCENES)
    return host, pt.DeviceScene(host.desc, 0, keepalive=host)


@pytest.fixture(scope="module")
def cornell():
    return open_scene()


def both_params(min_spp, max_spp, step, threshold):
    return pt.PtrAdaptiveParams(min_spp, max_spp, step, threshold), adaptive_ref.params(min_spp, max_spp, step, threshold)


# --------------------------------------------------------------------------- 1. the round kernels are the header's text
def check_round(w, h, min_max_step_thr, n_before, x, active, state, last=True):
    """One probe call against round_ref: state, next list and length bit for bit, nothing written past the length.  x [spp, len(active), 3]."""
    p_dev, p_ref = both_params(*min_max_step_thr)
    x4 = np.concatenate([x, np.full(x.shape[:2] + (1,), 9.0, np.float32)], axis=2)      # w is ignored
    got, nxt, count = pt.adaptive_debug_round(w, h, p_dev, n_before, x4, active, state, last_sub_pass=last)
    want, want_next, _ = adaptive_ref.round_ref(w, h, p_ref, n_before, x, active, state, last=last)
    for k in STATE_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (k, w, h, len(active))
    assert count == len(want_next) and np.array_equal(nxt[:count], want_next), (w, h, len(active), count, len(want_next))
    if last:
        assert (nxt[count:] == UNWRITTEN).all()
    return got, nxt[:count]


def noisy(spp, entries, seed):
    return np.random.default_rng(seed).uniform(0.05, 2.0, (spp, entries, 3)).astype(np.float32)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 45)])
def test_round_kernels_against_the_restatement(w, h):
    """67x45 = 3,015 pixels: 12 blocks of 256 with a ragged last one, waves that straddle kept and dropped runs.  The samples are
    lognormal with outliers, two rows of zeros and a NaN pixel; the threshold is the median of the restatement's dilated error, so
    about half the entries are kept."""
    pixels = w * h
    x = adaptive_ref.synthetic_samples(12, h, w).reshape(12, pixels, 3)
    order = adaptive_ref.pixel_order(w, h)
    zero = adaptive_ref.zero_state(pixels)
    _, _, big = adaptive_ref.round_ref(w, h, adaptive_ref.params(4, 12, 4, 0.0), 0, x[:4, order], order, zero)
    thr = float(np.median(big))
    lists = {"full": order, "one": order[pixels // 2:pixels // 2 + 1], "257": order[3:260], "every other": order[::2]}
    for name, active in lists.items():
        if active.size == 0:
            continue
        state, nxt = check_round(w, h, (4, 12, 4, thr), 0, x[:4, active], active, zero)
        if name == "full" and pixels > 1:
            assert 0 < nxt.size < pixels                      # a mixed keep pattern
        if nxt.size:                                           # a second round carries the state over; the third is clipped at maxSpp
            state, nxt2 = check_round(w, h, (4, 12, 4, thr), 4, x[4:8, nxt], nxt, state)
            if nxt2.size:
                state, nxt3 = check_round(w, h, (4, 12, 4, thr), 8, x[8:12, nxt2], nxt2, state)
                assert nxt3.size == 0 and (state["n"][nxt2] == 12).all()
    # all kept / none kept
    everywhere = noisy(4, pixels, 11)
    _, nxt = check_round(w, h, (4, 12, 4, 0.0), 0, everywhere, order, zero)
    assert np.array_equal(nxt, order)
    _, nxt = check_round(w, h, (4, 12, 4, 1e30), 0, everywhere, order, zero)
    assert nxt.size == 0
    _, nxt = check_round(w, h, (4, 4, 4, 0.0), 0, everywhere, order, zero)      # at maxSpp nobody goes on
    assert nxt.size == 0


def test_a_kept_run_across_a_block_boundary():
    w, h = 67, 45
    order = adaptive_ref.pixel_order(w, h)
    x = np.full((4, w * h, 3), 0.5, np.float32)
    x[:, 250:263] = noisy(4, 13, 12)                          # list entries 250 .. 262: blocks 0 and 1, waves 3 and 4
    _, nxt = check_round(w, h, (4, 8, 4, 0.01), 0, x, order, adaptive_ref.zero_state(w * h))
    kept = np.isin(order, nxt)
    assert kept[250:263].all() and 13 < nxt.size < 80 and not kept[:128].any()


def test_a_round_in_two_sub_passes_is_the_single_call():
    w, h = 67, 45
    active = adaptive_ref.pixel_order(w, h)[::2]
    x = adaptive_ref.synthetic_samples(6, h, w).reshape(6, w * h, 3)[:, active]
    zero = adaptive_ref.zero_state(w * h)
    one, next_one = check_round(w, h, (2, 16, 6, 0.05), 0, x, active, zero)
    half, same = check_round(w, h, (2, 16, 6, 0.05), 0, x[:4], active, zero, last=False)
    assert np.array_equal(same, active) and (half["e"] == 0).all()          # e is computed on the last sub-pass only
    two, next_two = check_round(w, h, (2, 16, 6, 0.05), 4, x[4:], active, half)
    assert np.array_equal(next_one, next_two) and all(np.array_equal(one[k], two[k], equal_nan=True) for k in STATE_KEYS)


# --------------------------------------------------------------------------- 2. the frame is the restatement of its own samples
W, H, MIN, STEP, MAX = 37, 21, 4, 4, 16


@pytest.fixture(scope="module")
def frame(cornell):
    """The 37x21 frame the tests below share: the samples of a uniform 16-spp frame (the existing probe), the restatement run on them
    with the threshold at the median of its own dilated first-round error, and the adaptive frame of the device."""
    host, dev = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    before, _ = dev.render_image(s, 5)
    samples = dev.debug_samples(s, MAX)
    first = adaptive_ref.adaptive_ref(samples[:MIN], adaptive_ref.params(MIN, MIN, STEP, 0.0))
    thr = float(np.median(first.E[0]))
    p_dev, p_ref = both_params(MIN, MAX, STEP, thr)
    want = adaptive_ref.adaptive_ref(samples, p_ref)
    got = dev.render_adaptive(s, p_dev)
    return s, p_dev, want, got, before


def test_the_input_splits_the_image(frame):
    """A condition on the input, from the restatement alone: with the threshold at the median, 20 % to 80 % of the pixels end at minSpp
    and at least three distinct counts occur."""
    _, _, want, _, _ = frame
    at_min = float((want.count == MIN).mean())
    print("pixels that end at %d spp: %.1f %%; counts %s" % (MIN, 100.0 * at_min, np.unique(want.count, return_counts=True)))
    assert 0.2 <= at_min <= 0.8 and len(np.unique(want.count)) >= 3


def test_frame_is_the_restatement_of_its_own_samples(frame):
    s, p, want, (rgb, cov, count, stats, info), _ = frame
    assert count.dtype == np.uint32 and np.array_equal(count, want.count)
    assert np.array_equal(rgb, want.rgb) and np.array_equal(cov, want.cov)
    assert info.rounds == want.rounds and info.active_counts() == want.active_after
    assert stats.samples == int(count.sum()) == info.totalSamples
    assert info.pixelsAtMax == int((count == MAX).sum())
    assert stats.totalSeconds > 0 and stats.traceLaunches > 0


# --------------------------------------------------------------------------- 3. every pixel is a uniform pixel
def test_every_pixel_is_the_uniform_pixel_of_its_count(cornell, frame):
    _, dev = cornell
    s, _, _, (rgb, cov, count, _, _), _ = frame
    for n in np.unique(count):
        u_rgb, u_cov, _ = dev.render_image_cov(s, int(n))          # one pass, through the existing entry point
        sel = count == n
        assert np.array_equal(rgb[sel], u_rgb[sel]) and np.array_equal(cov[sel], u_cov[sel]), int(n)


# --------------------------------------------------------------------------- 4. invariance
def test_frame_does_not_depend_on_how_it_is_rendered(cornell, frame):
    host, dev = cornell
    s, p, _, (rgb, cov, count, _, info), before = frame

    def same(out, what):
        assert np.array_equal(out[0], rgb) and np.array_equal(out[1], cov) and np.array_equal(out[2], count), what
        assert out[4].rounds == info.rounds and out[4].active_counts() == info.active_counts(), what

    same(dev.render_adaptive(s, p), "second run")
    assert np.array_equal(dev.render_image(s, 5)[0], before)      # the partition cache survived the adaptive frames

    def with_env(env, fresh_scene):
        os.environ.update(env)
        try:
            scene = open_scene()[1] if fresh_scene else dev       # the pool knobs are read when a scene is uploaded
            out = scene.render_adaptive(s, p)
            plain = scene.render_image(s, 5)[0]
            if fresh_scene:
                scene.close()
        finally:
            for k in env:
                del os.environ[k]
        same(out, env)
        return plain

    # PTR_MAX_ITEMS=1024: round 0's 777 x 4 accumulators arrive in sub-passes of one sample each
    for env, fresh in (({"PTR_POOL_SLOTS": "1024"}, True), ({"PTR_POOL_GROUPS": "1"}, True), ({"PTR_MAX_ITEMS": "1024"}, False)):
        plain = with_env(env, fresh)
        if "PTR_MAX_ITEMS" not in env:                            # (a frame of several passes sums in another order than one pass)
            assert np.array_equal(plain, before), env
    # the device entry point on a stream of torch's, into pre-filled buffers
    t_rgb = torch.full((H, W, 3), 7.0, device="cuda")
    t_cov = torch.full((H, W, 6), 7.0, device="cuda")
    t_count = torch.full((H, W), 7, device="cuda", dtype=torch.int32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        stats, dinfo = dev.render_adaptive_device(s, p, t_rgb.data_ptr(), t_cov.data_ptr(), t_count.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    same((t_rgb.cpu().numpy(), t_cov.cpu().numpy(), t_count.cpu().numpy().view(np.uint32), stats, dinfo), "device entry point")
    assert stats.samples == int(count.sum())
    # cov and count pointers null
    t_rgb.fill_(7.0)
    _, dinfo = dev.render_adaptive_device(s, p, t_rgb.data_ptr(), want_stats=False)
    torch.cuda.synchronize()
    assert np.array_equal(t_rgb.cpu().numpy(), rgb) and dinfo.rounds == info.rounds
    out = dev.render_adaptive(s, p, want_cov=False, want_count=False)
    assert np.array_equal(out[0], rgb) and out[1] is None and out[2] is None
    assert np.array_equal(dev.render_image(s, 5)[0], before)


# --------------------------------------------------------------------------- 5. limits
def test_limits(cornell):
    host, dev = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    # threshold 0 with max = min: one round, the uniform frame of minSpp
    rgb, cov, count, stats, info = dev.render_adaptive(s, pt.PtrAdaptiveParams(6, 6, 3, 0.0))
    u_rgb, u_cov, _ = dev.render_image_cov(s, 6)
    assert info.rounds == 1 and (count == 6).all() and np.array_equal(rgb, u_rgb) and np.array_equal(cov, u_cov)
    assert info.pixelsAtMax == W * H and stats.samples == 6 * W * H and info.active_counts() == [0]      # at maxSpp nobody goes on
    # the last round is clipped: 4, 4 + 5, 9 + 2
    rgb, cov, count, stats, info = dev.render_adaptive(s, pt.PtrAdaptiveParams(4, 11, 5, 0.05))
    assert set(np.unique(count)) <= {4, 9, 11} and count.max() == 11 and info.rounds == 3
    for n in np.unique(count):
        u_rgb, u_cov, _ = dev.render_image_cov(s, int(n))
        assert np.array_equal(rgb[count == n], u_rgb[count == n]) and np.array_equal(cov[count == n], u_cov[count == n])
    with pytest.raises(pt.PtrError, match="ptr_render_adaptive: .*minSpp"):
        dev.render_adaptive(s, pt.PtrAdaptiveParams(1, 8, 4, 0.05))


def test_pure_background_stops_at_the_first_round():
    """tests/golden/smoke.scene: two spheres under a solid sky; the top rows of the image see nothing else."""
    host, dev = open_scene("smoke.scene")
    s = host.settings_for(width=64, height=64, max_depth=4, seed=1337)
    rgb, cov, count, _, info = dev.render_adaptive(s, pt.PtrAdaptiveParams(4, 16, 4, 0.02))
    sky = (slice(0, 8), slice(None))
    assert (count[sky] == 4).all() and (cov[sky] == 0.0).all() and (rgb[sky] == rgb[0, 0]).all() and (rgb[0, 0] > 0).all()
    assert count.max() == 16 and info.rounds == 4                 # ... and the spheres do not
    dev.close()


# --------------------------------------------------------------------------- 6. with the denoiser, and the CLI
def test_adaptive_frame_under_the_denoiser_and_the_cli(cornell, tmp_path):
    host, dev = cornell
    s = host.settings_for(width=64, height=64, max_depth=4, seed=1337)
    first = adaptive_ref.adaptive_ref(dev.debug_samples(s, 4), adaptive_ref.params(4, 4, 4, 0.0))
    thr = float(np.float32(np.median(first.E[0])))                 # about half the pixels stop after the first round
    p = pt.PtrAdaptiveParams(4, 16, 4, thr)
    rgb, cov, count, _, info = dev.render_adaptive(s, p)
    assert 4 * 64 * 64 < int(count.sum()) < 16 * 64 * 64
    albedo, normal = dev.render_aovs(s, 0)
    filtered = pt.denoise(rgb, albedo, normal, cov=cov)
    assert np.isfinite(filtered).all() and not np.array_equal(filtered, rgb)
    common = [pt.CLI_PATH, "--scene=" + os.path.join(GOLDEN, "cornell_small_mesh.scene"), "--assets=" + SCENES, "--width=64", "--height=64",
              "--sppTotal=16", "--maxDepth=4", "--seed=1337", "--format=pfm", "--adaptive=%r" % thr, "--adaptiveMinSpp=4", "--adaptiveStep=4"]
    plain, denoised = tmp_path / "adaptive.pfm", tmp_path / "adaptive_denoised.pfm"
    r = subprocess.run(common + ["--output=" + str(plain), "--verbose"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pt.read_pfm(str(plain)), rgb)
    mean_spp = "%.2f spp on average" % (int(count.sum()) / (64.0 * 64.0))
    assert mean_spp in r.stdout and "%d rounds" % info.rounds in r.stdout and "adaptive: %d rounds" % info.rounds in r.stderr, r.stdout
    r = subprocess.run(common + ["--output=" + str(denoised), "--denoise", "--denoiseVariance=sample"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pt.read_pfm(str(denoised)), filtered)
