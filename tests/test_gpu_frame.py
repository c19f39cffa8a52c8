"""GPU tests of resumable frames (include/ptr_frame.h, csrc/kernels/frame.hip, csrc/host/frame.cpp): the frame without a scene against the
numpy restatement (tests/frame_ref.py) call by call, the frame continued against the frame rendered at once, resuming, the checkpoint,
independence from whatever else the scene renders, reset, the CLI's --snapshots, and the lines the three round loops print under
PTR_VERBOSE=launches.

Unless stated the scene is tests/golden/cornell_small_mesh.scene at 37x21, depth 4, seed 1337.  Everything is compared bit for bit."""
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import adaptive_ref
import frame_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(ROOT, "scenes")
STATE_KEYS = ("sum", "mean", "m", "n", "e")
W, H, MIN, STEP, MAX, MORE = 37, 21, 4, 4, 16, 24
# The threshold of the second refine is this quantile of the first round's dilated error.  On this scene it is 0 (more than a quarter of
# the pixels see the light or the background only and have no error at all), so the second refine takes every pixel with a noisy
# neighbour to 24: from the restatement on the scene's samples, 389 / 169 / 93 / 126 pixels hold 4 / 8 / 12 / 16 samples after the first
# refine, pixels resume from 4, 8 and 12, and S is a strict subset of L in the first three rounds (95, 264, 357 of 483).
QUANTILE = 0.25


def open_scene(name="cornell_small_mesh.scene"):
    host = pt.HostScene.load(os.path.join(GOLDEN, name), SCENES)
    return host, pt.DeviceScene(host.desc, 0, keepalive=host)


def both_params(min_spp, max_spp, step, threshold):
    return pt.PtrAdaptiveParams(min_spp, max_spp, step, threshold), adaptive_ref.params(min_spp, max_spp, step, threshold)


def thresholds(samples, quantile=QUANTILE):
    """The median and a lower quantile of the restatement's dilated error after the first MIN samples."""
    first = adaptive_ref.adaptive_ref(samples[:MIN], adaptive_ref.params(MIN, MIN, STEP, 0.0))
    return float(np.median(first.E[0])), float(np.quantile(first.E[0], quantile))


def same_state(got, want, what):
    for k in STATE_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (k, what)


def same_image(got, want, what):
    for a, b, name in zip(got, want, ("rgb", "cov", "count")):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (name, what)


def same_as_ref(frame, ref, what):
    same_state(frame.export_state(), ref.state, what)
    same_image(frame.resolve(), ref.resolve(), what)
    i = frame.info()
    n = ref.state["n"]
    assert (i.width, i.height, i.minCount, i.maxCount, i.totalSamples, i.uniform) == (ref.width, ref.height, n.min(), n.max(), int(n.sum()),
                                                                                       int(n.min() == n.max())), what


def same_info(info, want, what):
    assert info.rounds == want.rounds and info.active_counts() == want.active_after[:32], what
    assert info.totalSamples == want.total_samples and info.pixelsAtMax == want.pixels_at_max, what


# --------------------------------------------------------------------------- 1. without a scene, against the restatement
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 45)])
def test_sceneless_frame_against_the_restatement(w, h):
    """67x45 = 3,015 pixels: 12 blocks of 256 with a ragged last one, and classes that interleave inside waves (at the second refine S
    is a strict subset of L in three rounds: tests/test_frame_host.py)."""
    x = adaptive_ref.synthetic_samples(MORE, h, w)
    thr, thr2 = thresholds(x)
    frame, ref = pt.debug_frame(x), frame_ref.FrameRef(x)
    same_as_ref(frame, ref, "empty")
    for spp in (3, 1):
        stats = frame.accumulate(spp)
        ref.accumulate(spp)
        same_as_ref(frame, ref, "accumulate %d" % spp)
        assert stats.samples == spp * w * h
    for p, q in (both_params(MIN, MAX, STEP, thr), both_params(MIN, MORE, STEP, thr2)):
        stats, info = frame.refine(p)
        want = ref.refine(q)
        same_as_ref(frame, ref, "refine to %d" % p.maxSpp)
        same_info(info, want, "refine to %d" % p.maxSpp)
        assert stats.samples == want.total_samples
    if w * h > 1000:
        assert len(np.unique(ref.state["n"])) >= 4
    frame.close()
    # threshold 0: every pixel with a noisy neighbour goes to the end; 1e30, and maxSpp at the current count: nothing happens
    frame, ref = pt.debug_frame(x), frame_ref.FrameRef(x)
    frame.accumulate(MIN)
    ref.accumulate(MIN)
    for min_max_step_thr in ((MIN, MORE, STEP, 1e30), (MIN, MIN, STEP, 0.0)):
        before = frame.export_state()
        p, q = both_params(*min_max_step_thr)
        _, info = frame.refine(p)
        same_info(info, ref.refine(q), min_max_step_thr)
        assert info.rounds == 0 and info.totalSamples == 0
        same_state(frame.export_state(), before, min_max_step_thr)
    p, q = both_params(MIN, MORE, 5, 0.0)      # 4 + 5 + 5 + 5 + 5: the last round is not clipped here, the next case's is
    _, info = frame.refine(p)
    same_info(info, ref.refine(q), "threshold 0")
    same_as_ref(frame, ref, "threshold 0")
    assert set(np.unique(ref.state["n"])) <= {MIN, MORE} and info.pixelsAtMax == int((ref.state["n"] == MORE).sum())
    frame.close()
    frame, ref = pt.debug_frame(x), frame_ref.FrameRef(x)      # an empty frame: the first accumulate is the call's; 4, 4 + 7, 11 + 5
    p, q = both_params(MIN, MAX, 7, 0.0)
    _, info = frame.refine(p)
    same_info(info, ref.refine(q), "empty, clipped")
    same_as_ref(frame, ref, "empty, clipped")
    frame.close()


def test_what_a_frame_refuses():
    """The refusals that need a frame to exist: each returns 1 with the function's name, and the frame is as it was."""
    w, h = 5, 3
    x = adaptive_ref.synthetic_samples(8, h, w)
    frame, ref = pt.debug_frame(x), frame_ref.FrameRef(x)
    frame.accumulate(1)
    ref.accumulate(1)
    with pytest.raises(pt.PtrError, match="^ptr_frame_refine: .*2 samples"):
        frame.refine(pt.PtrAdaptiveParams(2, 8, 2, 0.0))
    frame.accumulate(3)
    ref.accumulate(3)
    with pytest.raises(pt.PtrError, match="^ptr_frame_accumulate: .*past"):
        frame.accumulate(5)
    with pytest.raises(pt.PtrError, match="^ptr_frame_refine: .*past"):
        frame.refine(pt.PtrAdaptiveParams(2, 9, 2, 0.0))
    with pytest.raises(pt.PtrError, match="^ptr_frame_accumulate: spp"):
        frame.accumulate(0)
    same_as_ref(frame, ref, "after the refusals")
    thr, _ = thresholds(x)
    frame.refine(pt.PtrAdaptiveParams(2, 8, 2, thr))
    ref.refine(adaptive_ref.params(2, 8, 2, thr))
    assert len(np.unique(ref.state["n"])) > 1 and not frame.info().uniform
    with pytest.raises(pt.PtrError, match="^ptr_frame_accumulate: .*not uniform"):
        frame.accumulate(1)
    same_as_ref(frame, ref, "after the non-uniform refusal")
    frame.close()
    with pytest.raises(pt.PtrError, match="closed"):
        frame.accumulate(1)


# --------------------------------------------------------------------------- the scene's frames
@pytest.fixture(scope="module")
def cornell():
    return open_scene()


@pytest.fixture(scope="module")
def resumed(cornell):
    """What the scene tests share: the samples of a uniform 24-spp frame (the existing probe), the thresholds, the restatement run on
    them - refine to 16 at the median, then to 24 at the lower quantile - and the device's frame after the same two calls, with its
    checkpoint between them."""
    host, dev = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    samples = dev.debug_samples(s, MORE)
    thr, thr2 = thresholds(samples)
    ref = frame_ref.FrameRef(samples)
    p1, q1 = both_params(MIN, MAX, STEP, thr)
    p2, q2 = both_params(MIN, MORE, STEP, thr2)
    want1 = ref.refine(q1)
    ref_first = {k: v.copy() for k, v in ref.state.items()}
    want2 = ref.refine(q2)
    frame = dev.frame(s)
    _, info1 = frame.refine(p1)
    checkpoint = frame.export_state()
    image1 = frame.resolve()
    _, info2 = frame.refine(p2)
    return dict(s=s, samples=samples, p1=p1, p2=p2, ref=ref, ref_first=ref_first, want1=want1, want2=want2, frame=frame, info1=info1, info2=info2,
                checkpoint=checkpoint, image1=image1, state=frame.export_state(), image=frame.resolve())


# --------------------------------------------------------------------------- 2. a frame continued is the frame rendered at once
def test_a_frame_continued_is_the_frame_rendered_at_once(cornell, resumed):
    host, dev = cornell
    s = resumed["s"]
    frame = dev.frame(s)
    frame.accumulate(3)
    stats = frame.accumulate(5)
    assert stats.samples == 5 * W * H and stats.totalSeconds > 0 and stats.traceLaunches > 0
    rgb, cov, count = frame.resolve()
    a_rgb, a_cov, a_count, _, _ = dev.render_adaptive(s, pt.PtrAdaptiveParams(8, 8, 1, 0.0))
    u_rgb, u_cov, _ = dev.render_image_cov(s, 8)
    assert (count == 8).all() and np.array_equal(count, a_count)
    assert np.array_equal(rgb, a_rgb) and np.array_equal(cov, a_cov) and np.array_equal(rgb, u_rgb) and np.array_equal(cov, u_cov)
    frame.close()
    # refine on an empty frame is render_adaptive
    a_rgb, a_cov, a_count, a_stats, a_info = dev.render_adaptive(s, resumed["p1"])
    same_image(resumed["image1"], (a_rgb, a_cov, a_count), "refine on an empty frame")
    info1 = resumed["info1"]
    assert info1.rounds == a_info.rounds and info1.active_counts() == a_info.active_counts()
    assert info1.totalSamples == a_info.totalSamples and info1.pixelsAtMax == a_info.pixelsAtMax
    assert 1 < info1.rounds and 0 < info1.active_counts()[0] < W * H


# --------------------------------------------------------------------------- 3. resume
def test_the_input_resumes_two_counts(resumed):
    """A condition on the input, from the restatement alone: the second refine picks up pixels that had stopped at two counts or more."""
    first, last = resumed["ref_first"]["n"], resumed["ref"].state["n"]
    went_on = np.unique(first[(last > first) & (first < MAX)])
    print("counts after the first refine %s; resumed from %s; at the end %s" % (np.unique(first, return_counts=True), went_on,
                                                                             np.unique(last, return_counts=True)))
    assert len(went_on) >= 2


def test_resumed_frame_is_the_restatement_and_every_pixel_is_uniform(cornell, resumed):
    _, dev = cornell
    ref = resumed["ref"]
    same_state(resumed["checkpoint"], resumed["ref_first"], "first refine")
    same_info(resumed["info1"], resumed["want1"], "first refine")
    same_state(resumed["state"], ref.state, "second refine")
    same_image(resumed["image"], ref.resolve(), "second refine")
    same_info(resumed["info2"], resumed["want2"], "second refine")
    rgb, cov, count = resumed["image"]
    for n in np.unique(count):
        u_rgb, u_cov, _ = dev.render_image_cov(resumed["s"], int(n))          # one pass, through the existing entry point
        sel = count == n
        assert np.array_equal(rgb[sel], u_rgb[sel]) and np.array_equal(cov[sel], u_cov[sel]), int(n)


# --------------------------------------------------------------------------- 4. checkpoint
def test_checkpoint(cornell, resumed):
    host, dev = cornell
    first = dev.frame(resumed["s"])
    first.refine(resumed["p1"])
    saved = first.export_state()
    first.close()
    same_state(saved, resumed["checkpoint"], "the checkpoint")
    again = dev.frame(resumed["s"])
    again.import_state(saved)
    i = again.info()
    assert (i.minCount, i.maxCount, i.totalSamples, i.uniform) == (MIN, MAX, int(saved["n"].sum()), 0)
    _, info = again.refine(resumed["p2"])
    same_state(again.export_state(), resumed["state"], "continued from the checkpoint")
    same_image(again.resolve(), resumed["image"], "continued from the checkpoint")
    assert info.rounds == resumed["info2"].rounds and info.active_counts() == resumed["info2"].active_counts()
    again.close()


# --------------------------------------------------------------------------- 5. independence
def test_frame_does_not_depend_on_what_else_the_scene_renders(cornell, resumed):
    host, dev = cornell
    s, p1, p2 = resumed["s"], resumed["p1"], resumed["p2"]
    before = dev.render_image(s, 5)[0]
    a, b = dev.frame(s), dev.frame(s)
    a.refine(p1)
    b.accumulate(6)
    dev.render_adaptive(s, pt.PtrAdaptiveParams(2, 9, 3, 0.01))
    assert np.array_equal(dev.render_image(s, 5)[0], before)
    same_state(a.export_state(), resumed["checkpoint"], "after other renders")
    a.refine(p2)
    b.accumulate(2)
    same_state(a.export_state(), resumed["state"], "two frames, other renders between the calls")
    u_rgb, u_cov, _ = dev.render_image_cov(s, 8)
    rgb, cov, count = b.resolve()
    assert np.array_equal(rgb, u_rgb) and np.array_equal(cov, u_cov) and (count == 8).all()
    b.close()

    def with_env(env, fresh_scene):
        os.environ.update(env)
        try:
            scene = open_scene()[1] if fresh_scene else dev       # the pool knobs are read when a scene is uploaded
            frame = scene.frame(s)
            frame.refine(p1)
            frame.refine(p2)
            state, image = frame.export_state(), frame.resolve()
            frame.close()
            if fresh_scene:
                scene.close()
        finally:
            for k in env:
                del os.environ[k]
        same_state(state, resumed["state"], env)
        same_image(image, resumed["image"], env)

    # PTR_MAX_ITEMS=1024: the first accumulate's 777 x 4 accumulators arrive in sub-passes of one sample each
    with_env({"PTR_MAX_ITEMS": "1024"}, False)
    with_env({"PTR_POOL_SLOTS": "1024"}, True)
    # the device entry point on a stream of torch's, into pre-filled buffers; cov and count null
    t_rgb = torch.full((H, W, 3), 7.0, device="cuda")
    t_cov = torch.full((H, W, 6), 7.0, device="cuda")
    t_count = torch.full((H, W), 7, device="cuda", dtype=torch.int32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        a.resolve_device(t_rgb.data_ptr(), t_cov.data_ptr(), t_count.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    same_image((t_rgb.cpu().numpy(), t_cov.cpu().numpy(), t_count.cpu().numpy().view(np.uint32)), resumed["image"], "resolve_device")
    t_rgb.fill_(7.0)
    with torch.cuda.stream(stream):
        a.resolve_device(t_rgb.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(t_rgb.cpu().numpy(), resumed["image"][0])
    out = a.resolve(want_cov=False, want_count=False)
    assert np.array_equal(out[0], resumed["image"][0]) and out[1] is None and out[2] is None
    same_state(a.export_state(), resumed["state"], "resolved three times")
    a.close()


# --------------------------------------------------------------------------- 6. reset
def test_reset(cornell, resumed):
    host, dev = cornell
    s = resumed["s"]
    frame = dev.frame(s)
    frame.refine(resumed["p1"])
    frame.reset()
    i = frame.info()
    assert (i.minCount, i.maxCount, i.totalSamples, i.uniform) == (0, 0, 0, 1)
    same_state(frame.export_state(), adaptive_ref.zero_state(W * H), "after reset")
    frame.refine(resumed["p1"])
    frame.refine(resumed["p2"])
    same_state(frame.export_state(), resumed["state"], "rendered again")
    other = host.settings_for(width=W + 1, height=H, max_depth=4, seed=1337)
    with pytest.raises(pt.PtrError, match="^ptr_frame_reset: "):
        frame.reset(other)
    same_state(frame.export_state(), resumed["state"], "after the refused reset")
    moved = s.copy()      # settings of the same size replace the stored ones
    moved.seed = 1338
    frame.reset(moved)
    frame.accumulate(4)
    rgb, cov, _ = frame.resolve()
    u_rgb, u_cov, _ = dev.render_image_cov(moved, 4)
    assert np.array_equal(rgb, u_rgb) and np.array_equal(cov, u_cov) and not np.array_equal(rgb, dev.render_image(s, 4)[0])
    frame.close()


# --------------------------------------------------------------------------- 7. the CLI
def test_cli_snapshots(tmp_path):
    common = [pt.CLI_PATH, "--scene=" + os.path.join(GOLDEN, "cornell_small_mesh.scene"), "--assets=" + SCENES, "--width=64", "--height=64",
              "--maxDepth=4", "--seed=1337", "--format=pfm"]
    out = tmp_path / "series.pfm"
    r = subprocess.run(common + ["--sppTotal=16", "--snapshots=4,8", "--output=" + str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Rendered 16 spp" in r.stdout and "Snapshot at 4 spp" in r.stdout and "Snapshot at 8 spp" in r.stdout
    for n, path in ((4, tmp_path / "series.4.pfm"), (8, tmp_path / "series.8.pfm"), (16, out)):
        alone = tmp_path / ("alone_%d.pfm" % n)
        r = subprocess.run(common + ["--sppTotal=%d" % n, "--output=" + str(alone)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(pt.read_pfm(str(path)), pt.read_pfm(str(alone))), n
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("series")) == ["series.4.pfm", "series.8.pfm", "series.pfm"]


# --------------------------------------------------------------------------- 8. the timed path of the three round loops
# The child of test_verbose_lines_of_the_three_loops: argv = root, the two thresholds.  The knobs are read once per process, so the timed
# path needs a process of its own.
VERBOSE_CHILD = """
import importlib, json, os, sys
root, thr, thr2 = sys.argv[1], float(sys.argv[2]), float(sys.argv[3])
sys.path.insert(0, root)
pt = importlib.import_module("metal-pathtracer-arm64_amd")
host = pt.HostScene.load(os.path.join(root, "tests", "golden", "cornell_small_mesh.scene"), os.path.join(root, "scenes"))
dev = pt.DeviceScene(host.desc, 0, keepalive=host)
s = host.settings_for(width=%d, height=%d, max_depth=4, seed=1337)
p1, p2 = pt.PtrAdaptiveParams(%d, %d, %d, thr), pt.PtrAdaptiveParams(%d, %d, %d, thr2)
out = {}
def note(name, info):
    out[name] = dict(rounds=int(info.rounds), active=info.active_counts())
note("adaptive", dev.render_adaptive(s, p1)[4])
frame = dev.frame(s)
note("refine1", frame.refine(p1)[1])
note("refine2", frame.refine(p2)[1])
frame.close()
multi = pt.render_multi_adaptive(host.desc, s, p1, device_ids=[0, 0])
note("multi", multi["info"])
out["multi_count"] = multi["count"].tolist()
mf = pt.multi_frame(host.desc, s, device_ids=[0, 0])
for name, p in (("mf_refine1", p1), ("mf_refine2", p2)):
    sys.stderr.write("[child] %%s begins\\n" %% name)
    sys.stderr.flush()
    info = mf.refine(p)[1]
    note(name, info)
    out[name]["total"] = int(info.totalSamples)
mf.close()
print(json.dumps(out))
""" % (W, H, MIN, MAX, STEP, MIN, MORE, STEP)
# the expressions tools/adaptive_cost.py, tools/frame_cost.py, tools/multi_adaptive_cost.py and tools/multi_frame_cost.py parse the lines with
ADAPTIVE_LINE = r"\[adaptive\] .*: (\d+) active x (\d+) spp; update ([0-9.]+) ms, select \+ compact ([0-9.]+) ms"
FRAME_LINE = r"\[frame\] round (\d+): class (\d+), (\d+) of (\d+) active x (\d+) spp; minimum \+ split ([0-9.]+) ms, select \+ merge ([0-9.]+) ms"
MULTI_LINE = r"\[multi\] partition (\d+) round (\d+): halo (\d+) bytes each way; pack \+ copy ([0-9.]+) ms, copy \+ unpack ([0-9.]+) ms"
MULTI_FRAME_LINE = (r"\[multi-frame\] partition (\d+) round (\d+): class (\d+), (\d+) entries x (\d+) spp; halo (\d+) bytes each way; "
                    r"pack \+ copy ([0-9.]+) ms, copy \+ unpack ([0-9.]+) ms")


def test_verbose_lines_of_the_three_loops(resumed):
    """PTR_VERBOSE=launches in a fresh process: ptr_render_adaptive, two refines of a frame and a two-partition frame on one device print
    one line per round each, with the counts the calls report; so do the same two refines of a resumable two-partition frame, per
    partition.  777 x 4 accumulators fit one pass, so no round is split."""
    env = dict(os.environ, PTR_VERBOSE="launches")
    r = subprocess.run([sys.executable, "-c", VERBOSE_CHILD, ROOT, repr(float(resumed["p1"].threshold)), repr(float(resumed["p2"].threshold))],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    lines = r.stderr.splitlines()

    def parsed(pattern, ints):
        rows = [m.groups() for m in (re.search(pattern, l) for l in lines) if m]
        for row in rows:
            assert all(float(ms) >= 0.0 for ms in row[ints:]), row
        return [tuple(int(v) for v in row[:ints]) for row in rows]

    def round_spp(n):
        return MIN if n == 0 else min(STEP, MAX - n)

    # [adaptive]: one line per round, with the list the round starts with and its samples
    a = got["adaptive"]
    assert a["rounds"] == resumed["info1"].rounds and a["active"] == resumed["info1"].active_counts()
    rows = parsed(ADAPTIVE_LINE, 2)
    print("[adaptive]", rows)
    n, want = 0, []
    for i in range(a["rounds"]):
        want.append((W * H if i == 0 else a["active"][i - 1], round_spp(n)))
        n += round_spp(n)
    assert rows == want
    # [frame]: one line per round beyond the one that ends with the first list (the empty frame's first samples)
    r1, r2 = got["refine1"], got["refine2"]
    assert (r1["rounds"], r1["active"]) == (a["rounds"], a["active"])
    assert (r2["rounds"], r2["active"]) == (resumed["info2"].rounds, resumed["info2"].active_counts())
    rows = parsed(FRAME_LINE, 5)
    print("[frame]", rows)
    assert len(rows) == r1["rounds"] - 1 + r2["rounds"]
    first, second = rows[:r1["rounds"] - 1], rows[r1["rounds"] - 1:]
    assert [row[0] for row in first] == list(range(1, r1["rounds"])) and [row[0] for row in second] == list(range(r2["rounds"]))
    for rnd, cls, in_class, active, spp in rows:
        assert 1 <= spp <= STEP and 1 <= in_class <= active <= W * H and cls % STEP == 0 and MIN <= cls < MORE
    for rnd, cls, in_class, active, spp in first:      # an empty frame: S = L, the class is the round's common count
        assert (cls, in_class, active, spp) == (MIN + (rnd - 1) * STEP, r1["active"][rnd - 1], r1["active"][rnd - 1], round_spp(cls))
    for rnd, cls, in_class, active, spp in second[1:]:
        assert active == r2["active"][rnd - 1]
    assert [row[1] for row in second] == sorted(row[1] for row in second)      # the lowest class first
    # [multi]: one line per partition and round in which the partition's list is not empty, i.e. one of its pixels ends above the
    # count the round starts at (partition q owns the 8-row bands b with b % 2 == q)
    m = got["multi"]
    assert (m["rounds"], m["active"]) == (a["rounds"], a["active"])
    rows = parsed(MULTI_LINE, 3)
    print("[multi]", rows)
    count = np.array(got["multi_count"])
    band = np.arange(H) // 8
    want, n = set(), 0
    for rnd in range(m["rounds"]):
        want |= {(q, rnd) for q in (0, 1) if (count[band % 2 == q] > n).any()}
        n += round_spp(n)
    assert len(rows) == len(want) and {row[:2] for row in rows} == want
    assert len(want) == 2 * m["rounds"]      # on this scene both partitions stay active to the end
    bands = [int((band % 2 == q)[::8].sum()) for q in (0, 1)]
    assert all(halo == bands[q] * 2 * W * 4 for q, _, halo in rows)
    # [multi-frame]: the two refines on a two-partition frame; at most one line per partition and round in which the partition's S_p
    # is not empty, with the round's class, |S_p| and samples.  The calls are the single-device frame's.
    marks = [i for i, l in enumerate(lines) if l.startswith("[child] mf_refine")]
    assert len(marks) == 2
    for name, single, begin, end, before in (("mf_refine1", r1, marks[0], marks[1], W * H * MIN), ("mf_refine2", r2, marks[1], len(lines), 0)):
        call = got[name]
        assert (call["rounds"], call["active"]) == (single["rounds"], single["active"]), name
        rows = [m.groups() for m in (re.search(MULTI_FRAME_LINE, l) for l in lines[begin:end]) if m]
        assert all(float(ms) >= 0.0 for row in rows for ms in row[6:]), name
        rows = [tuple(int(v) for v in row[:6]) for row in rows]
        print("[multi-frame]", name, rows)
        assert len({row[:2] for row in rows}) == len(rows), name
        assert all(entries >= 1 and 1 <= spp <= STEP for _, _, _, entries, spp, _ in rows), name
        classes = {}
        for _, rnd, cls, _, _, _ in rows:
            assert classes.setdefault(rnd, cls) == cls, (name, rnd)
        assert [classes[rnd] for rnd in sorted(classes)] == sorted(classes.values()), name
        assert before + sum(entries * spp for _, _, _, entries, spp, _ in rows) == call["total"], name
