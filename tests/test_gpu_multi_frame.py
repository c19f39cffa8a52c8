"""GPU tests of resumable frames on several devices (include/ptr_multi_frame.h, csrc/host/multi_frame.cpp, k_multi_state_pack /
k_multi_state_unpack of csrc/kernels/multi.hip): the frame without a scene against the single-device numpy restatement
(tests/frame_ref.py) call by call, the scene's frame against a single-device Frame step by step, the checkpoint across device counts,
sub-passes, and the refusals that need a frame to exist.

An id that repeats lets one GPU run every partition and the exchange between them; -(id + 1) forces the staged gather of a resolve.
Everything is compared bit for bit."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import adaptive_ref
import frame_ref
import multi_frame_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(ROOT, "scenes")
STATE_KEYS = ("sum", "mean", "m", "n", "e")
MIN, STEP, MAX, MORE = 4, 4, 16, 24
ID_LISTS = [[0], [0, 0], [0, 0, 0], [0] * 9, [0, -1, -1]]


def thresholds(samples, quantile=0.25):
    """tests/test_gpu_frame.py's: the median and a lower quantile of the restatement's dilated error after the first MIN samples."""
    first = adaptive_ref.adaptive_ref(samples[:MIN], adaptive_ref.params(MIN, MIN, STEP, 0.0))
    return float(np.median(first.E[0])), float(np.quantile(first.E[0], quantile))


def same_state(got, want, what):
    for k in STATE_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (k, what)


def same_image(got, want, what):
    for a, b, name in zip(got, want, ("rgb", "cov", "count")):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (name, what)


def frame_info(frame):
    i = frame.info()
    return (i.width, i.height, i.minCount, i.maxCount, i.totalSamples, i.uniform)


def adaptive_info(info):
    return (int(info.rounds), info.active_counts(), int(info.totalSamples), int(info.pixelsAtMax))


# --------------------------------------------------------------------------- 1. without a scene, against the single-device restatement
# A script is a list of calls: ("accumulate", spp) or ("refine", (min, max, step, threshold)).  The restatement runs a script once per
# input; what it holds after every call is kept and never changed.
def script_a(thr, thr2):
    return [("accumulate", 3), ("accumulate", 1), ("refine", (MIN, MAX, STEP, thr)), ("refine", (MIN, MORE, STEP, thr2))]


def script_thresholds(thr, thr2):
    """threshold 1e30, and maxSpp at the current count: nothing happens; threshold 0 with 4 + 5 + 5 + 5 + 5: every pixel with a noisy
    neighbour goes to the end"""
    return [("accumulate", MIN), ("refine", (MIN, MORE, STEP, 1e30)), ("refine", (MIN, MIN, STEP, 0.0)), ("refine", (MIN, MORE, 5, 0.0))]


def script_clipped(thr, thr2):
    """an empty frame: the first accumulate is the call's; 4, 4 + 7, 11 + 5: the last round is clipped"""
    return [("refine", (MIN, MAX, 7, 0.0))]


SCRIPTS = {"a": script_a, "thresholds": script_thresholds, "clipped": script_clipped}
_samples, _expected = {}, {}


def samples_of(kind, w, h):
    if (kind, w, h) not in _samples:
        x = adaptive_ref.synthetic_samples(MORE, h, w) if kind == "synthetic" else multi_frame_ref.quiet_band_samples(MORE, h, w)
        _samples[(kind, w, h)] = (x, thresholds(x))
    return _samples[(kind, w, h)]


def snapshot(ref, info=None):
    n = ref.state["n"]
    return dict(state={k: v.copy() for k, v in ref.state.items()}, image=ref.resolve(),
                frame_info=(ref.width, ref.height, n.min(), n.max(), int(n.sum()), int(n.min() == n.max())),
                info=None if info is None else (info.rounds, info.active_after[:32], info.total_samples, info.pixels_at_max))


def expected(kind, w, h, script):
    """[(call, what the single-device restatement holds after it)], the empty frame first"""
    key = (kind, w, h, script)
    if key not in _expected:
        x, (thr, thr2) = samples_of(kind, w, h)
        ref = frame_ref.FrameRef(x)
        steps = [(("empty", None), snapshot(ref))]
        for call in SCRIPTS[script](thr, thr2):
            if call[0] == "accumulate":
                ref.accumulate(call[1])
                steps.append((call, snapshot(ref)))
            else:
                steps.append((call, snapshot(ref, ref.refine(adaptive_ref.params(*call[1])))))
        _expected[key] = steps
    return _expected[key]


def same_as_snapshot(frame, want, what):
    same_state(frame.export_state(), want["state"], what)
    same_image(frame.resolve(), want["image"], what)
    assert frame_info(frame) == want["frame_info"], what


def replay(frame, steps, what):
    for (op, arg), want in steps:
        if op == "accumulate":
            stats = frame.accumulate(arg)
            assert stats.samples == arg * want["frame_info"][0] * want["frame_info"][1], (what, op, arg)
        elif op == "refine":
            stats, info = frame.refine(pt.PtrAdaptiveParams(*arg))
            assert adaptive_info(info) == want["info"], (what, op, arg)
            assert stats.samples == want["info"][2], (what, op, arg)
            multi = frame.multi_info()
            assert sum(multi.partSamples[:multi.parts]) == want["info"][2], (what, op, arg)
        same_as_snapshot(frame, want, (what, op, arg))


SCENELESS = ([("synthetic", 1, 1, ids) for ids in ID_LISTS] + [("synthetic", 5, 3, ids) for ids in ID_LISTS] +
             [("synthetic", 67, 45, ids) for ids in ID_LISTS + [[0] * 7]] + [("synthetic", 130, 70, ids) for ids in ([0, 0], [0] * 9)] +
             [("quiet band", 67, 45, ids) for ids in ([0, 0], [0] * 7)])


@pytest.mark.parametrize("kind,w,h,ids", SCENELESS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_sceneless_frame_against_the_single_device_restatement(kind, w, h, ids):
    """Script A, then the threshold-0, threshold-1e30 and clipped-last-round cases of tests/test_gpu_frame.py: after every call the
    exported state, the resolve, the info and the PtrAdaptiveInfo are those of the single-device restatement.  67x45 has a ragged last
    band and, with seven ids, more partitions than bands; on the quiet-band input (tests/test_multi_frame_host.py) the partition that
    owns band 1 alone has an empty S_p beside a non-empty L_p in three rounds."""
    x, _ = samples_of(kind, w, h)
    for script in SCRIPTS:
        frame = pt.debug_multi_frame(x, ids)
        assert frame.multi_info().parts == len(ids)
        replay(frame, expected(kind, w, h, script), (kind, w, h, ids, script))
        frame.close()
    if w * h > 1000:
        assert len(np.unique(expected(kind, w, h, "a")[-1][1]["state"]["n"])) >= 4
    unchanged = expected(kind, w, h, "thresholds")
    assert unchanged[2][1]["info"][0] == 0 and unchanged[3][1]["info"][0] == 0      # (the restatement's own: nothing happened)


# --------------------------------------------------------------------------- 2. the scene's frame against a single-device Frame
W, H = 88, 72


@pytest.fixture(scope="module")
def cornell():
    host = pt.HostScene.load(os.path.join(GOLDEN, "cornell_small_mesh.scene"), SCENES)
    return host, pt.DeviceScene(host.desc, 0, keepalive=host)


@pytest.fixture(scope="module")
def series(cornell):
    """The single-device Frame after each step of accumulate 4 -> refine(median) -> refine(0.25 quantile, maxSpp 24), computed once:
    its state, resolve, infos; the denoised image of its last step; the scene's feature buffers."""
    host, dev = cornell
    s = host.settings_for(width=W, height=H, max_depth=4, seed=1337)
    thr, thr2 = thresholds(dev.debug_samples(s, MIN))
    p1, p2 = pt.PtrAdaptiveParams(MIN, MAX, STEP, thr), pt.PtrAdaptiveParams(MIN, MORE, STEP, thr2)
    frame = dev.frame(s)
    steps = []
    for call in (("accumulate", MIN), ("refine", p1), ("refine", p2)):
        info = None
        if call[0] == "accumulate":
            frame.accumulate(call[1])
        else:
            info = adaptive_info(frame.refine(call[1])[1])
        steps.append((call, dict(state=frame.export_state(), image=frame.resolve(), frame_info=frame_info(frame), info=info)))
    frame.close()
    albedo, normal = dev.render_aovs(s)
    return dict(s=s, p1=p1, p2=p2, steps=steps, albedo=albedo, normal=normal, denoised=denoise_chain(steps[-1][1]["image"], albedo, normal, None))


def denoise_chain(image, albedo, normal, frame):
    """ptr_denoise_cov_device on device buffers: the image's (frame None: uploaded from the host) or what frame.resolve_device wrote."""
    t_rgb = torch.full((H, W, 3), 7.0, device="cuda")
    t_cov = torch.full((H, W, 6), 7.0, device="cuda")
    if frame is None:
        t_rgb.copy_(torch.from_numpy(image[0]))
        t_cov.copy_(torch.from_numpy(image[1]))
    else:
        frame.resolve_device(t_rgb.data_ptr(), t_cov.data_ptr())
    t_albedo, t_normal = torch.from_numpy(albedo).cuda(), torch.from_numpy(normal).cuda()
    t_out = torch.zeros((H, W, 3), device="cuda")
    torch.cuda.synchronize()
    pt.denoise_device(t_rgb.data_ptr(), t_albedo.data_ptr(), t_normal.data_ptr(), W, H, d_out=t_out.data_ptr(), d_cov=t_cov.data_ptr())
    torch.cuda.synchronize()
    return t_rgb.cpu().numpy(), t_cov.cpu().numpy(), t_out.cpu().numpy()


def test_the_scene_input_mixes_counts(series):
    """A condition on the input, from the single-device Frame alone: the series ends with at least 4 distinct counts, and both refines
    ran rounds."""
    counts = np.unique(series["steps"][-1][1]["state"]["n"], return_counts=True)
    print("counts at the end %s; infos %s %s" % (counts, series["steps"][1][1]["info"], series["steps"][2][1]["info"]))
    assert len(counts[0]) >= 4 and series["steps"][1][1]["info"][0] > 1 and series["steps"][2][1]["info"][0] > 1


@pytest.mark.parametrize("ids", ID_LISTS, ids=lambda v: "x".join(map(str, v)))
def test_scene_frame_is_the_single_device_frame(cornell, series, ids):
    host, _ = cornell
    frame = pt.multi_frame(host.desc, series["s"], device_ids=ids)
    for (op, arg), want in series["steps"]:
        if op == "accumulate":
            frame.accumulate(arg)
        else:
            assert adaptive_info(frame.refine(arg)[1]) == want["info"], (ids, op)
        same_as_snapshot(frame, want, (ids, op))
    rgb, cov, count, albedo, normal = frame.resolve(want_aovs=True)
    same_image((rgb, cov, count), series["steps"][-1][1]["image"], "resolve with feature buffers")
    assert np.array_equal(albedo, series["albedo"]) and np.array_equal(normal, series["normal"])
    multi = frame.multi_info()
    assert (multi.parts, multi.stagedParts) == (len(ids), sum(1 for i in ids if i < 0))
    # resolve_device followed by denoise_cov_device is the single-device chain
    got = denoise_chain(None, albedo, normal, frame)
    for a, b, name in zip(got, series["denoised"], ("rgb", "cov", "denoised")):
        assert np.array_equal(a, b, equal_nan=True), (ids, name)
    out = frame.resolve(want_cov=False, want_count=False)
    assert np.array_equal(out[0], rgb) and out[1] is None and out[2] is None
    same_state(frame.export_state(), series["steps"][-1][1]["state"], "resolved four times")
    # reset, then the series again in one call each
    frame.reset()
    assert frame_info(frame) == (W, H, 0, 0, 0, 1)
    same_state(frame.export_state(), adaptive_ref.zero_state(W * H), "after reset")
    frame.refine(series["p1"])
    same_state(frame.export_state(), series["steps"][1][1]["state"], "refine on the empty frame")
    frame.close()


# --------------------------------------------------------------------------- 3. the checkpoint across device counts
def test_checkpoint_across_device_counts(cornell, series):
    host, dev = cornell
    s, p1, p2 = series["s"], series["p1"], series["p2"]
    mid, last = series["steps"][1][1], series["steps"][2][1]
    three = pt.multi_frame(host.desc, s, device_ids=[0, 0, 0])
    three.accumulate(MIN)
    three.refine(p1)
    saved = three.export_state()
    same_state(saved, mid["state"], "the checkpoint of three partitions")
    targets = [("two partitions", pt.multi_frame(host.desc, s, device_ids=[0, 0])), ("nine partitions", pt.multi_frame(host.desc, s, device_ids=[0] * 9)),
               ("a plain frame", dev.frame(s))]
    # ... and the reverse: the single-device frame's checkpoint into three partitions that hold something else by now
    three.refine(p2)
    three.import_state(mid["state"])
    targets.append(("from a plain frame into three partitions", three))
    for what, frame in targets:
        if frame is not three:
            frame.import_state(saved)
        assert frame_info(frame) == mid["frame_info"], what
        same_state(frame.export_state(), mid["state"], what)
        assert adaptive_info(frame.refine(p2)[1]) == last["info"], what
        same_state(frame.export_state(), last["state"], what)
        same_image(frame.resolve()[:3], last["image"], what)
        frame.close()


@pytest.mark.parametrize("w,h,ids", [(5, 3, [0, 0, 0]), (67, 45, [0, 0, 0]), (67, 45, [0] * 7)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_pack_and_unpack_round_trip_any_words(w, h, ids):
    """A state of distinct words in every plane, NaNs among them, through import (k_multi_state_unpack) and export (k_multi_state_pack)
    unchanged; both sizes have a ragged last band."""
    pixels = w * h
    rng = np.random.default_rng(11)
    state = {k: (rng.integers(1, 0x7F000000, size=(pixels, cols) if cols else pixels, dtype=np.uint32)) for k, cols, _ in pt.FRAME_STATE}
    for k in ("sum", "mean", "m", "e"):
        state[k].reshape(-1)[::5] = np.uint32(0x7FC00000) | (state[k].reshape(-1)[::5] & np.uint32(0x3FFFFF))      # quiet NaNs with payloads
    state["n"] = (np.arange(pixels, dtype=np.uint32) % 13) + 2
    as_floats = {k: v if k == "n" else v.view(np.float32) for k, v in state.items()}
    frame = pt.debug_multi_frame(np.zeros((2, h, w, 3), np.float32), ids)
    frame.import_state(as_floats)
    back = frame.export_state()
    for k in STATE_KEYS:
        assert np.array_equal(back[k].view(np.uint32), as_floats[k].view(np.uint32)), k
    i = frame.info()
    assert (i.minCount, i.maxCount, i.totalSamples, i.uniform) == (2, int(state["n"].max()), int(state["n"].sum()), 0)
    frame.close()


# --------------------------------------------------------------------------- 4. sub-passes
# The child of test_sub_passes_give_the_same_bits: argv = root, the two thresholds, the output file.  The knobs are read once per
# process, so PTR_MAX_ITEMS needs a process of its own.
SUB_PASS_CHILD = """
import importlib, os, sys
import numpy as np
root, thr, thr2, out = sys.argv[1], float(sys.argv[2]), float(sys.argv[3]), sys.argv[4]
sys.path[:0] = [root, os.path.join(root, "tests")]
import adaptive_ref
pt = importlib.import_module("metal-pathtracer-arm64_amd")
frame = pt.debug_multi_frame(adaptive_ref.synthetic_samples(%d, 45, 67), [0, 0, 0])
frame.accumulate(3)
frame.accumulate(1)
frame.refine(pt.PtrAdaptiveParams(%d, %d, %d, thr))
frame.refine(pt.PtrAdaptiveParams(%d, %d, %d, thr2))
np.savez(out, **frame.export_state())
frame.close()
""" % (MORE, MIN, MAX, STEP, MIN, MORE, STEP)


def test_sub_passes_give_the_same_bits(tmp_path):
    """PTR_MAX_ITEMS=1024 in a fresh process: a partition of 67x45 on three holds 1,072 or 871 pixels, so every round of more than one
    sample arrives in sub-passes of one sample, and the halo goes out behind the last one only."""
    _, (thr, thr2) = samples_of("synthetic", 67, 45)
    out = str(tmp_path / "state.npz")
    r = subprocess.run([sys.executable, "-c", SUB_PASS_CHILD, ROOT, repr(thr), repr(thr2), out], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PTR_MAX_ITEMS="1024"))
    assert r.returncode == 0, r.stderr[-2000:]
    same_state(dict(np.load(out)), expected("synthetic", 67, 45, "a")[-1][1]["state"], "PTR_MAX_ITEMS=1024")


# --------------------------------------------------------------------------- 5. the refusals that need a device
def test_device_count_rules(cornell):
    host, _ = cornell
    visible = pt.device_count()
    s = host.settings_for(width=16, height=24, max_depth=2, seed=1)
    lib = pt.load_library()
    handle, err = C.c_void_p(), C.create_string_buffer(256)
    rc = lib.ptr_multi_frame_create(C.byref(host.desc), C.byref(s), visible + 1, C.byref(handle), err, len(err))
    assert rc == 2 and err.value.decode().startswith("ptr_multi_frame_create:") and "visible" in err.value.decode() and not handle.value
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_debug_create_on: no such HIP device"):
        pt.multi_frame(host.desc, s, device_ids=[0, visible])
    frame = pt.multi_frame(host.desc, s)                       # all visible devices, never more partitions than the three bands
    assert frame.multi_info().parts == min(visible, 3)
    frame.close()
    one_band = host.settings_for(width=16, height=8, max_depth=2, seed=1)
    frame = pt.multi_frame(host.desc, one_band, n_devices=visible)
    assert frame.multi_info().parts == 1
    frame.close()


def test_what_a_multi_frame_refuses():
    """Each refusal returns 1 with the function's name, and the frame is as it was.  9x19: three bands on three partitions."""
    w, h = 9, 19
    x = adaptive_ref.synthetic_samples(8, h, w)
    frame, ref = pt.debug_multi_frame(x, [0, 0, 0]), frame_ref.FrameRef(x)
    frame.accumulate(1)
    ref.accumulate(1)
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_refine: .*2 samples"):
        frame.refine(pt.PtrAdaptiveParams(2, 8, 2, 0.0))
    frame.accumulate(3)
    ref.accumulate(3)
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_accumulate: .*past"):
        frame.accumulate(5)
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_refine: .*past"):
        frame.refine(pt.PtrAdaptiveParams(2, 9, 2, 0.0))
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_accumulate: spp"):
        frame.accumulate(0)
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_resolve: .*feature buffers"):
        frame.resolve(want_aovs=True)
    other = pt.PtrSettings()
    other.width, other.height = w + 1, h
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_reset: "):
        frame.reset(other)
    same_as_snapshot(frame, snapshot(ref), "after the refusals")
    thr, _ = thresholds(x)
    frame.refine(pt.PtrAdaptiveParams(2, 8, 2, thr))
    ref.refine(adaptive_ref.params(2, 8, 2, thr))
    assert len(np.unique(ref.state["n"])) > 1 and not frame.info().uniform
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_accumulate: .*not uniform"):
        frame.accumulate(1)
    same_as_snapshot(frame, snapshot(ref), "after the non-uniform refusal")
    frame.close()
    with pytest.raises(pt.PtrError, match="closed"):
        frame.accumulate(1)
