"""CPU tests of the adaptive-sampling surface (include/ptr_adaptive.h): the exported functions and their ctypes table, the argument checks,
the CLI flags, and the numpy restatement the GPU tests compare the kernels with (tests/adaptive_ref.py) on synthetic samples."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref
import stats_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_adaptive_header():
    text = open(os.path.join(ROOT, "include", "ptr_adaptive.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text):
        found[name] = (ret, 0 if args.strip() in ("", "void") else args.count(",") + 1)
    assert set(found) == set(pt.ADAPTIVE_SYMBOLS) and len(found) == len(pt.ADAPTIVE_SYMBOLS) == 4
    assert found == {"ptr_adaptive_default_params": ("void", 2), "ptr_render_adaptive_device": ("int", 11), "ptr_render_adaptive": ("int", 10),
                     "ptr_adaptive_debug_round": ("int", 18)}
    lib = pt.load_library()
    for name, (ret, count) in found.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, name
        assert fn.restype is (C.c_int if ret == "int" else None), name


def test_adaptive_symbols_are_in_no_other_table():
    others = set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS) | set(pt.POST_SYMBOLS) | set(pt.STATS_SYMBOLS)
    assert not set(pt.ADAPTIVE_SYMBOLS) & others
    assert len(set(pt.ADAPTIVE_SYMBOLS)) == len(pt.ADAPTIVE_SYMBOLS)


def test_structs_and_defaults_match_the_header():
    assert C.sizeof(pt.PtrAdaptiveParams) == 16 and C.sizeof(pt.PtrAdaptiveInfo) == 16 + 4 * 32
    p = pt.PtrAdaptiveParams.defaults(64)
    assert (p.minSpp, p.maxSpp, p.stepSpp) == (8, 64, 8) and p.threshold == np.float32(0.05)
    assert pt.PtrAdaptiveParams.defaults(3).maxSpp == 8          # never below minSpp
    assert pt.PtrAdaptiveParams.defaults(64, stepSpp=3).stepSpp == 3


# --------------------------------------------------------------------------- bad arguments
def _params(min_spp=4, max_spp=16, step=4, threshold=0.1):
    return pt.PtrAdaptiveParams(min_spp, max_spp, step, threshold)


BAD_PARAMS = [_params(min_spp=1), _params(min_spp=0), _params(min_spp=8, max_spp=7), _params(step=0), _params(threshold=-0.5),
              _params(threshold=math.nan), _params(threshold=math.inf)]


def _render_call(name, scene, settings, params, rgb, cov, count):
    """`scene` is a made-up handle: a bad argument must be refused before anything looks behind it."""
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    sp = None if settings is None else C.byref(settings)
    pp = None if params is None else C.byref(params)
    if name == "ptr_render_adaptive":
        fp = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
        rc = lib.ptr_render_adaptive(scene, sp, pp, fp(rgb, C.c_float), fp(cov, C.c_float), fp(count, C.c_uint32), None, None, err, len(err))
    else:
        vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        rc = lib.ptr_render_adaptive_device(scene, sp, pp, vp(rgb), vp(cov), vp(count), None, None, None, err, len(err))
    return rc, err.value.decode()


@pytest.mark.parametrize("name", ["ptr_render_adaptive", "ptr_render_adaptive_device"])
def test_bad_render_arguments_are_refused_by_name(name):
    settings = pt.PtrSettings()
    settings.width, settings.height, settings.maxDepth = 8, 8, 2
    no_width, no_height = settings.copy(), settings.copy()
    no_width.width, no_height.height = 0, 0
    rgb, cov, count = np.full((8, 8, 3), 7.0, np.float32), np.full((8, 8, 6), 7.0, np.float32), np.full((8, 8), 7, np.uint32)
    scene = C.c_void_p(0x1000)      # never dereferenced by a refused call
    good = _params()
    cases = [(None, settings, good, rgb, cov, count), (scene, None, good, rgb, cov, count), (scene, settings, None, rgb, cov, count),
             (scene, settings, good, None, cov, count), (scene, no_width, good, rgb, cov, count), (scene, no_height, good, rgb, cov, count)]
    cases += [(scene, settings, p, rgb, cov, count) for p in BAD_PARAMS]
    for case in cases:
        rc, message = _render_call(name, *case)
        assert rc == 1 and message.startswith(name + ":"), (rc, message)
    assert "minSpp" in _render_call(name, scene, settings, _params(min_spp=1), rgb, cov, count)[1]
    assert "threshold" in _render_call(name, scene, settings, _params(threshold=math.nan), rgb, cov, count)[1]
    assert (rgb == 7.0).all() and (cov == 7.0).all() and (count == 7).all()


def _round_call(width, height, params, n_before, samples, active, state, nxt, drop=None):
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    count = C.c_uint32(77)
    args = [width, height, None if params is None else C.byref(params), n_before, samples.shape[0], 1, u(active), active.size, f(samples),
            f(state["sum"]), f(state["mean"]), f(state["m"]), u(state["n"]), f(state["e"]), u(nxt), C.byref(count)]
    if drop is not None:
        args[drop] = None
    rc = lib.ptr_adaptive_debug_round(*args, err, len(err))
    return rc, err.value.decode(), count.value


def test_bad_probe_arguments_are_refused_by_name():
    w, h = 4, 3
    state = adaptive_ref.zero_state(w * h)
    samples = np.ones((4, w * h, 4), np.float32)
    active = np.arange(w * h, dtype=np.uint32)
    nxt = np.full(w * h, 7, np.uint32)
    good = _params()
    name = "ptr_adaptive_debug_round"
    for drop in (2, 6, 8, 9, 10, 11, 12, 13, 14, 15):       # each pointer in turn
        rc, message, _ = _round_call(w, h, good, 0, samples, active, state, nxt, drop=drop)
        assert rc == 1 and message.startswith(name + ":"), (drop, rc, message)
    for p in BAD_PARAMS:
        rc, message, _ = _round_call(w, h, p, 0, samples, active, state, nxt)
        assert rc == 1 and message.startswith(name + ":"), (rc, message)
    outside = active.copy()
    outside[5] = w * h               # a pixel outside the image is refused, not read
    bad = [(0, h, good, 0, samples, active), (w, 0, good, 0, samples, active), (w, h, good, 0, samples, outside),
           (w, h, good, 14, samples, active),                  # 14 + 4 samples > maxSpp
           (w, h, good, 0, samples[:0], active), (w, h, good, 0, samples, active[:0])]
    for case in bad:
        rc, message, _ = _round_call(*case, state, nxt)
        assert rc == 1 and message.startswith(name + ":"), (rc, message)
    assert (nxt == 7).all() and all((v == 0).all() for v in state.values())


def test_adaptive_fails_loudly_without_gpu():
    if pt.device_count() > 0:
        pytest.skip("a GPU is present")
    settings = pt.PtrSettings()
    settings.width, settings.height, settings.maxDepth = 8, 8, 2
    rgb, cov, count = np.full((8, 8, 3), 7.0, np.float32), np.full((8, 8, 6), 7.0, np.float32), np.full((8, 8), 7, np.uint32)
    for name in ("ptr_render_adaptive", "ptr_render_adaptive_device"):
        rc, message = _render_call(name, C.c_void_p(0x1000), settings, _params(), rgb, cov, count)
        assert rc == 2 and message.startswith(name + ":") and "no CPU fallback" in message, (name, rc, message)
    w, h = 4, 3
    state = adaptive_ref.zero_state(w * h)
    nxt = np.full(w * h, 7, np.uint32)
    rc, message, _ = _round_call(w, h, _params(), 0, np.ones((4, w * h, 4), np.float32), np.arange(w * h, dtype=np.uint32), state, nxt)
    assert rc == 2 and "no CPU fallback" in message
    assert (rgb == 7.0).all() and (nxt == 7).all()
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.adaptive_debug_round(w, h, _params(), 0, np.ones((4, w * h, 4), np.float32), np.arange(w * h), state)
    host = pt.HostScene.load(os.path.join(GOLDEN, "smoke.scene"))
    with pytest.raises(pt.PtrError, match="no HIP device|no such HIP device"):
        pt.DeviceScene(host.desc).render_adaptive(host.settings_for(width=8, height=8), _params())


def test_cli_documents_and_checks_the_adaptive_flags():
    helped = subprocess.run([pt.CLI_PATH, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert helped.returncode == 0
    for flag in ("--adaptive[=<threshold>]", "--adaptiveMinSpp=<n>", "--adaptiveStep=<n>"):
        assert flag in helped.stdout, flag
    scene = os.path.join(GOLDEN, "smoke.scene")
    run = lambda *flags: subprocess.run([pt.CLI_PATH, "--scene=" + scene, *flags], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    usage_errors = [("--adaptive=-1",), ("--adaptive=nan",), ("--adaptive=inf",), ("--adaptive=abc",), ("--adaptive=0.1x",), ("--adaptive=",),
                    ("--adaptive", "--adaptiveMinSpp=1"), ("--adaptive", "--adaptiveStep=0"), ("--adaptiveMinSpp=4",), ("--adaptiveStep=4",),
                    ("--adaptive", "--sppTotal=4"), ("--adaptive", "--adaptiveMinSpp=16", "--sppTotal=8")]
    for flags in usage_errors:
        res = run(*flags)
        assert res.returncode != 0 and "daptive" in res.stdout and "Usage:" in res.stdout, flags
    for devices in ("--devices=2", "--devices=0"):
        res = run("--adaptive", devices)
        assert res.returncode != 0 and "--adaptive" in res.stdout and "device" in res.stdout, devices
        assert "Usage:" not in res.stdout and "HIP" not in res.stdout      # refused with a message, before any device call


# --------------------------------------------------------------------------- the restatement on synthetic samples
def test_constant_samples_stop_at_the_first_round():
    x = np.full((16, 9, 11, 3), 0.375, np.float32)
    x[..., 1] = 1.5
    r = adaptive_ref.adaptive_ref(x, adaptive_ref.params(4, 16, 4, 0.01))
    assert r.rounds == 1 and r.active_after == [0] and (r.count == 4).all()
    assert np.array_equal(r.rgb, x[0]) and (r.cov == 0.0).all()
    assert np.array_equal(r.lists[0], adaptive_ref.pixel_order(11, 9)) and sorted(r.lists[0]) == list(range(99))


def test_first_list_is_the_blocked_order():
    order = adaptive_ref.pixel_order(11, 9)
    assert list(order[:8]) == list(range(8)) and order[8] == 11 and order[64] == 8 and order[67] == 11 + 8
    assert order[88] == 8 * 11                                   # the second band starts after the two blocks of the first


def test_one_noisy_pixel_keeps_exactly_its_neighbours():
    rng = np.random.default_rng(5)
    x = np.full((16, 9, 11, 3), 0.5, np.float32)
    x[:, 4, 6] = rng.uniform(0.0, 4.0, (16, 3)).astype(np.float32)
    x[:, 0, 0] = rng.uniform(0.0, 4.0, (16, 3)).astype(np.float32)      # a corner: its window has four pixels
    r = adaptive_ref.adaptive_ref(x, adaptive_ref.params(4, 16, 4, 0.01))
    want = np.full((9, 11), 4, np.uint32)
    want[3:6, 5:8] = 16
    want[0:2, 0:2] = 16
    assert np.array_equal(r.count, want) and r.active_after == [13, 13, 13, 0] and r.rounds == 4
    kept = [p for p in r.lists[0] if want.reshape(-1)[p] == 16]
    assert list(r.lists[1]) == kept and list(r.lists[3]) == kept       # stable: the first list's order


def test_threshold_zero_runs_every_pixel_with_a_noisy_neighbour_to_the_end():
    rng = np.random.default_rng(6)
    x = np.zeros((12, 8, 8, 3), np.float32)
    x[:, :, :4] = rng.uniform(0.1, 1.0, (12, 8, 4, 3)).astype(np.float32)
    r = adaptive_ref.adaptive_ref(x, adaptive_ref.params(2, 12, 3, 0.0))
    want = np.full((8, 8), 2, np.uint32)
    want[:, :5] = 12                                              # the noisy half and the column beside it
    assert np.array_equal(r.count, want) and (r.cov[:, 5:] == 0).all() and (r.rgb[:, 4:] == 0).all()


def test_a_nan_sample_does_not_spread():
    x = np.full((8, 5, 5, 3), 0.25, np.float32)
    x[1, 2, 2, 0] = np.nan
    r = adaptive_ref.adaptive_ref(x, adaptive_ref.params(4, 8, 4, 0.01))
    assert (r.count == 4).all() and r.rounds == 1                 # neither the pixel nor its neighbours go on
    assert (r.e[0] == 0).all() and (r.E[0] == 0).all() and np.isnan(r.rgb[2, 2, 0]) and np.isfinite(np.delete(r.rgb.reshape(-1, 3), 12, 0)).all()
    # a NaN in the error map itself is never taken by the dilation
    e = np.zeros(25, np.float32)
    e[12], e[13] = np.nan, 0.5
    big = adaptive_ref.dilate(e, 5, 5).reshape(5, 5)
    assert np.isfinite(big).all() and big[2, 2] == 0.5 and big[1, 1] == 0 and big[2, 4] == 0.5


def test_the_last_round_is_clipped():
    x = adaptive_ref.synthetic_samples(11, 6, 7)
    r = adaptive_ref.adaptive_ref(x, adaptive_ref.params(4, 11, 5, 0.05))
    assert set(np.unique(r.count)) <= {4, 9, 11} and r.count.max() == 11 and r.rounds == 3


def test_every_pixel_is_the_uniform_pixel_of_its_count():
    h, w = 13, 10
    x = adaptive_ref.synthetic_samples(16, h, w)
    finite = np.isfinite(x).all(axis=(0, 3))
    E0 = adaptive_ref.adaptive_ref(x[:4], adaptive_ref.params(4, 4, 4, 0.0)).E[0]
    r = adaptive_ref.adaptive_ref(x, adaptive_ref.params(4, 16, 4, float(np.median(E0))))
    assert len(np.unique(r.count)) >= 3 and r.count.min() == 4
    for n in np.unique(r.count):
        sel = (r.count == n) & finite
        total = np.zeros((h, w, 3), np.float32)
        for c in range(n):
            total = total + x[c]
        assert np.array_equal(r.rgb[sel], (total / np.float32(n))[sel]), n
        assert np.array_equal(r.cov[sel], stats_ref.welford32(x[:n])[sel]), n
    assert np.isnan(r.rgb[~finite]).all()
    assert int(r.count.sum()) == 4 * sum(len(l) for l in r.lists)        # every round here has four samples


def test_round_ref_in_two_sub_passes_is_the_single_call():
    w, h = 7, 6
    x = adaptive_ref.synthetic_samples(6, h, w).reshape(6, h * w, 3)
    p = adaptive_ref.params(2, 16, 6, 0.05)
    active = adaptive_ref.pixel_order(w, h)[::2]
    st0 = adaptive_ref.zero_state(w * h)
    one, next_one, _ = adaptive_ref.round_ref(w, h, p, 0, x[:, active], active, st0)
    half, same, none = adaptive_ref.round_ref(w, h, p, 0, x[:4, active], active, st0, last=False)
    assert none is None and np.array_equal(same, active) and (half["e"] == 0).all()
    two, next_two, _ = adaptive_ref.round_ref(w, h, p, 4, x[4:, active], active, half)
    assert np.array_equal(next_one, next_two) and all(np.array_equal(one[k], two[k], equal_nan=True) for k in one)
    assert (one["n"][active] == 6).all() and one["n"].sum() == 6 * active.size
