"""CPU tests of the surface of resumable frames on several devices (include/ptr_multi_frame.h): the exported functions and their ctypes
table, the argument checks, and the numpy restatement the GPU tests stand beside (tests/multi_frame_ref.py) - that with the true halo
it is the single-device restatement (tests/frame_ref.py) bit for bit for every number of partitions and is NOT with a wrong halo, on
the inputs the GPU tests use, and that a checkpoint does not depend on the number of partitions.

The refusals that need a frame to exist - the device-count rules, a non-uniform frame given to accumulate, a pixel below 2 samples
given to refine, another size given to reset - are in tests/test_gpu_multi_frame.py: a frame is created on devices only."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import adaptive_ref
import frame_ref
import multi_frame_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = {"ptr_multi_frame_create": ("int", 6), "ptr_multi_frame_release": ("void", 1), "ptr_multi_frame_reset": ("int", 4),
          "ptr_multi_frame_accumulate": ("int", 5), "ptr_multi_frame_refine": ("int", 6), "ptr_multi_frame_resolve": ("int", 8),
          "ptr_multi_frame_resolve_device": ("int", 7), "ptr_multi_frame_info": ("int", 3), "ptr_multi_frame_export": ("int", 8),
          "ptr_multi_frame_import": ("int", 8), "ptr_multi_frame_debug_create_on": ("int", 7), "ptr_multi_frame_debug_create": ("int", 9)}
SIZES = [(1, 1), (5, 3), (67, 45), (130, 70)]
PARTS = [1, 2, 3, 6, 9, 11]
WRONG = ("none", "stale_start", "no_publish_after_accumulate")
STATE_KEYS = ("sum", "mean", "m", "n", "e")


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_multi_frame_header():
    text = open(os.path.join(ROOT, "include", "ptr_multi_frame.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text):
        found[name] = (ret, 0 if args.strip() in ("", "void") else args.count(",") + 1)
    assert set(found) == set(pt.MULTI_FRAME_SYMBOLS) and len(found) == len(pt.MULTI_FRAME_SYMBOLS) == 12
    assert found == COUNTS
    lib = pt.load_library()
    for name, (ret, count) in found.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, name
        assert fn.restype is (C.c_int if ret == "int" else None), name


def test_multi_frame_symbols_are_in_no_other_table_and_every_table_keeps_its_size():
    tables = (pt.ABI_SYMBOLS, pt.DEBUG_SYMBOLS, pt.POST_SYMBOLS, pt.STATS_SYMBOLS, pt.ADAPTIVE_SYMBOLS, pt.MULTI_SYMBOLS, pt.FRAME_SYMBOLS)
    others = set().union(*map(set, tables))
    assert not set(pt.MULTI_FRAME_SYMBOLS) & others
    assert len(set(pt.MULTI_FRAME_SYMBOLS)) == len(pt.MULTI_FRAME_SYMBOLS)
    assert (len(pt.ABI_SYMBOLS) + len(pt.DEBUG_SYMBOLS), len(pt.POST_SYMBOLS), len(pt.STATS_SYMBOLS), len(pt.ADAPTIVE_SYMBOLS), len(pt.MULTI_SYMBOLS),
            len(pt.FRAME_SYMBOLS)) == (48, 4, 5, 4, 5, 11)


def test_python_mirrors_frame():
    """MultiFrame has Frame's calls under Frame's names."""
    for name in ("accumulate", "refine", "resolve", "resolve_device", "export_state", "import_state", "info", "reset", "close"):
        assert callable(getattr(pt.MultiFrame, name)) and callable(getattr(pt.Frame, name)), name
    assert callable(pt.multi_frame) and callable(pt.debug_multi_frame)


# --------------------------------------------------------------------------- bad arguments
def _call(name, *args):
    err = C.create_string_buffer(256)
    rc = getattr(pt.load_library(), name)(*args, err, len(err))
    return rc, err.value.decode()


def _refused(name, *args):
    rc, message = _call(name, *args)
    assert rc == 1 and message.startswith(name + ":"), (name, rc, message)
    return message


def _settings(width=8, height=8):
    s = pt.PtrSettings()
    s.width, s.height, s.maxDepth = width, height, 2
    return s


def _ids(*ids):
    return (C.c_int * max(len(ids), 1))(*ids)


def test_bad_arguments_are_refused_by_name():
    """`frame` is a made-up handle and the scene description is never looked into: a bad argument must be refused before anything
    looks behind them."""
    frame = C.c_void_p(0x1000)
    desc, good = C.byref(pt.PtrSceneDesc()), _settings()
    huge = _settings(0x10000, 0x10000)
    out = C.c_void_p()
    for args in ((None, C.byref(good), 1, C.byref(out)), (desc, None, 1, C.byref(out)), (desc, C.byref(good), 1, None),
                 (desc, C.byref(_settings(0, 8)), 1, C.byref(out)), (desc, C.byref(_settings(8, 0)), 1, C.byref(out)), (desc, C.byref(huge), 1, C.byref(out)),
                 (desc, C.byref(good), 65, C.byref(out))):
        _refused("ptr_multi_frame_create", *args)
    two = _ids(0, 0)
    for args in ((None, C.byref(good), two, 2, C.byref(out)), (desc, None, two, 2, C.byref(out)), (desc, C.byref(good), None, 2, C.byref(out)),
                 (desc, C.byref(good), two, 2, None), (desc, C.byref(_settings(0, 8)), two, 2, C.byref(out)), (desc, C.byref(good), two, 0, C.byref(out)),
                 (desc, C.byref(good), _ids(*([0] * 65)), 65, C.byref(out))):
        _refused("ptr_multi_frame_debug_create_on", *args)
    samples = np.ones((2, 8, 8, 4), np.float32)
    sp = samples.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((8, 8, None, 2, two, 2, C.byref(out)), (8, 8, sp, 2, None, 2, C.byref(out)), (8, 8, sp, 2, two, 2, None), (0, 8, sp, 2, two, 2, C.byref(out)),
                 (8, 0, sp, 2, two, 2, C.byref(out)), (8, 8, sp, 0, two, 2, C.byref(out)), (0x10000, 0x10000, sp, 2, two, 2, C.byref(out)),
                 (8, 8, sp, 2, two, 0, C.byref(out)), (8, 8, sp, 2, _ids(*([0] * 65)), 65, C.byref(out))):
        _refused("ptr_multi_frame_debug_create", *args)
    assert not out.value
    _refused("ptr_multi_frame_reset", None, C.byref(good))
    _refused("ptr_multi_frame_accumulate", None, 4, None)
    assert "spp" in _refused("ptr_multi_frame_accumulate", frame, 0, None)
    params = pt.PtrAdaptiveParams(4, 16, 4, 0.1)
    _refused("ptr_multi_frame_refine", None, C.byref(params), None, None)
    _refused("ptr_multi_frame_refine", frame, None, None, None)
    rgb = np.full((8, 8, 3), 7.0, np.float32)
    fp = rgb.ctypes.data_as(C.POINTER(C.c_float))
    _refused("ptr_multi_frame_resolve", None, fp, None, None, None, None)
    _refused("ptr_multi_frame_resolve", frame, None, None, None, None, None)
    _refused("ptr_multi_frame_resolve_device", None, C.c_void_p(rgb.ctypes.data), None, None, None)
    _refused("ptr_multi_frame_resolve_device", frame, None, None, None, None)
    st = {k: np.full_like(v, 7) for k, v in adaptive_ref.zero_state(64).items()}
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    full = [frame, f(st["sum"]), f(st["mean"]), f(st["m"]), u(st["n"]), f(st["e"])]
    for name in ("ptr_multi_frame_export", "ptr_multi_frame_import"):
        for drop in range(6):
            args = list(full)
            args[drop] = None
            _refused(name, *args)
    info = pt.PtrFrameInfo()
    lib = pt.load_library()
    assert lib.ptr_multi_frame_info(None, C.byref(info), None) == 1 and lib.ptr_multi_frame_info(frame, None, None) == 1
    lib.ptr_multi_frame_release(None)
    assert (rgb == 7.0).all() and all((v == 7).all() for v in st.values())      # the buffers are untouched


def test_bad_refine_parameters_are_refused_by_name():
    """Behind a handle that is never dereferenced: the parameters are checked before the frame is looked at."""
    bad = [pt.PtrAdaptiveParams(1, 16, 4, 0.1), pt.PtrAdaptiveParams(0, 16, 4, 0.1), pt.PtrAdaptiveParams(8, 7, 4, 0.1),
           pt.PtrAdaptiveParams(4, 16, 0, 0.1), pt.PtrAdaptiveParams(4, 16, 4, -0.5), pt.PtrAdaptiveParams(4, 16, 4, math.nan),
           pt.PtrAdaptiveParams(4, 16, 4, math.inf)]
    for p in bad:
        _refused("ptr_multi_frame_refine", C.c_void_p(0x1000), C.byref(p), None, None)
    assert "minSpp" in _refused("ptr_multi_frame_refine", C.c_void_p(0x1000), C.byref(bad[0]), None, None)


def test_multi_frames_fail_loudly_without_gpu():
    if pt.device_count() > 0:
        pytest.skip("a GPU is present")
    out = C.c_void_p()
    desc, good = C.byref(pt.PtrSceneDesc()), _settings()
    samples = np.ones((2, 8, 8, 4), np.float32)
    sp = samples.ctypes.data_as(C.POINTER(C.c_float))
    for name, args in (("ptr_multi_frame_create", (desc, C.byref(good), 0, C.byref(out))),
                       ("ptr_multi_frame_debug_create_on", (desc, C.byref(good), _ids(0, 0), 2, C.byref(out))),
                       ("ptr_multi_frame_debug_create", (8, 8, sp, 2, _ids(0, 0), 2, C.byref(out)))):
        rc, message = _call(name, *args)
        assert rc == 2 and message.startswith(name + ":") and "no CPU fallback" in message and not out.value, name
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.debug_multi_frame(samples, [0, 0])
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.multi_frame(pt.PtrSceneDesc(), good, device_ids=[0])


# --------------------------------------------------------------------------- the restatement
def thresholds(samples):
    """tests/test_gpu_frame.py's: the median and the 0.25 quantile of the dilated error after the first four samples."""
    first = adaptive_ref.adaptive_ref(samples[:4], adaptive_ref.params(4, 4, 4, 0.0))
    return float(np.median(first.E[0])), float(np.quantile(first.E[0], 0.25))


def script_a(ref, thr, thr2, between=None):
    """accumulate 3, accumulate 1, refine(4, 16, 4, median), refine(4, 24, 4, the 0.25 quantile); between(ref) runs after the first
    refine and may hand back another frame to go on with.  Returns (frame, the two infos)."""
    ref.accumulate(3)
    ref.accumulate(1)
    info1 = ref.refine(adaptive_ref.params(4, 16, 4, thr))
    if between:
        ref = between(ref)
    info2 = ref.refine(adaptive_ref.params(4, 24, 4, thr2))
    return ref, (info1, info2)


_inputs = {}


def single(w, h):
    """Script A on the single-device restatement, computed once per size and left unchanged."""
    if (w, h) not in _inputs:
        x = adaptive_ref.synthetic_samples(24, h, w)
        thr, thr2 = thresholds(x)
        ref, infos = script_a(frame_ref.FrameRef(x), thr, thr2)
        _inputs[(w, h)] = (x, thr, thr2, ref, infos)
    return _inputs[(w, h)]


def same_state(got, want, what):
    for k in STATE_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (k, what)


def same_info(got, want, what):
    assert vars(got) == vars(want), what


@pytest.mark.parametrize("w,h", SIZES)
def test_true_halo_is_the_single_device_frame_for_every_number_of_partitions(w, h):
    x, thr, thr2, want, want_infos = single(w, h)
    for parts in PARTS:
        ref, infos = script_a(multi_frame_ref.MultiFrameRef(x, parts), thr, thr2)
        same_state(ref.state, want.state, parts)
        for a, b in zip(infos, want_infos):
            same_info(a, b, parts)
        assert ref.log == want.log, parts
        for a, b in zip(ref.resolve(), want.resolve()):
            assert np.array_equal(a, b, equal_nan=True), parts


def idle_pairs(ref):
    """(partition, round) pairs with an empty S_p while L_p is not empty"""
    return sum(1 for rnd in ref.parts_log for n_s, n_l in rnd if n_s == 0 and n_l > 0)


@pytest.mark.parametrize("w,h", [(67, 45), (130, 70)])
def test_the_input_discriminates(w, h):
    """Conditions on the input, from the restatements alone: each wrong halo changes at least 20 final counts for every P >= 2, and at
    least 4 distinct counts occur.  Measured: 209 / 28 / 28 counts at 67x45 and 610 / 200 / 200 at 130x70 for none / stale_start /
    no_publish_after_accumulate, the same for every P >= 2 (every band edge is a partition edge); the counts 4, 8, 12, 16, 20, 24.
    On these two inputs no partition ever has an empty S_p beside a non-empty L_p (every band holds pixels of every class):
    test_a_partition_idles_with_a_list holds that condition on an input made for it."""
    x, thr, thr2, want, _ = single(w, h)
    counts = sorted(int(v) for v in np.unique(want.state["n"]))
    changed, idle = {}, {}
    for parts in PARTS[1:]:
        for halo in WRONG:
            ref, _ = script_a(multi_frame_ref.MultiFrameRef(x, parts, halo), thr, thr2)
            changed[(halo, parts)] = int((ref.state["n"] != want.state["n"]).sum())
        idle[parts] = idle_pairs(script_a(multi_frame_ref.MultiFrameRef(x, parts), thr, thr2)[0])
    print("%dx%d: counts %s; final counts changed by a wrong halo %s; (partition, round) pairs with an empty S_p and a non-empty L_p %s"
          % (w, h, counts, changed, idle))
    assert len(counts) >= 4
    assert all(v >= 20 for v in changed.values()), changed


def test_a_partition_idles_with_a_list():
    """The third condition on the input: in at least one round some partition has an empty S_p while its L_p is not empty.  Script A on
    multi_frame_ref.quiet_band_samples at 67x45: with P = 6, 7, 9 or 11 partition 1 owns band 1 alone.  The true variant is the
    single-device frame there too, and each wrong halo still changes final counts (measured at P = 7: 136 / 15 / 15; the bound of 20
    belongs to the two inputs of test_the_input_discriminates, this one only has to tell the variants apart at all)."""
    w, h = 67, 45
    x = multi_frame_ref.quiet_band_samples(24, h, w)
    thr, thr2 = thresholds(x)
    want, want_infos = script_a(frame_ref.FrameRef(x), thr, thr2)
    idle = {}
    for parts in (2, 6, 7, 9, 11):
        ref, infos = script_a(multi_frame_ref.MultiFrameRef(x, parts), thr, thr2)
        same_state(ref.state, want.state, parts)
        same_info(infos[1], want_infos[1], parts)
        idle[parts] = idle_pairs(ref)
    changed = {halo: int((script_a(multi_frame_ref.MultiFrameRef(x, 7, halo), thr, thr2)[0].state["n"] != want.state["n"]).sum()) for halo in WRONG}
    print("quiet band: idle (partition, round) pairs %s; counts %s; changed by a wrong halo at P = 7 %s" % (idle, np.unique(want.state["n"], return_counts=True), changed))
    assert all(idle[parts] > 0 for parts in (6, 7, 9, 11)), idle
    assert all(v > 0 for v in changed.values()), changed


@pytest.mark.parametrize("w,h", [(5, 3), (67, 45)])
def test_checkpoint_law_in_the_restatement(w, h):
    """Export at P = 3 after the first refine, import at Q = 1, 2, 9 (and into the single-device restatement), continue: the frame
    that was never interrupted."""
    x, thr, thr2, want, want_infos = single(w, h)
    for q in (1, 2, 9, None):
        def move(ref):
            saved = ref.export_state()
            other = frame_ref.FrameRef(x) if q is None else multi_frame_ref.MultiFrameRef(x, q)
            if q is None:
                other.state = {k: v.copy() for k, v in saved.items()}
            else:
                other.import_state(saved)
            return other
        ref, infos = script_a(multi_frame_ref.MultiFrameRef(x, 3), thr, thr2, between=move)
        same_state(ref.state, want.state, q)
        same_info(infos[1], want_infos[1], q)
    # ... and the reverse: from the single-device restatement into three partitions
    def split(ref):
        other = multi_frame_ref.MultiFrameRef(x, 3)
        other.import_state(ref.state)
        return other
    ref, infos = script_a(frame_ref.FrameRef(x), thr, thr2, between=split)
    same_state(ref.state, want.state, "reverse")
    same_info(infos[1], want_infos[1], "reverse")
