"""CPU tests of the multi-device surface of include/ptr_multi.h: the exported functions and their ctypes table, the argument checks, the
partitioned numpy restatement (tests/multi_ref.py) - that it is the single-device restatement with the true halo and is NOT with a missing
or a stale one, on the inputs the GPU tests use - and the round barrier's stand-alone program."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref
import multi_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = {"ptr_render_multi_cov": 13, "ptr_render_multi_adaptive": 15, "ptr_multi_debug_cov_on": 13, "ptr_multi_debug_adaptive_on": 15,
          "ptr_multi_debug_adaptive_frame": 12}
# the plain frame (include/ptr_abi.h and its test-only variant of include/ptr_debug.h) goes through the same driver and the same checks
PLAIN = ("ptr_render_multi", "ptr_debug_render_multi_on")


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_multi_header():
    text = open(os.path.join(ROOT, "include", "ptr_multi.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text):
        found[name] = (ret, 0 if args.strip() in ("", "void") else args.count(",") + 1)
    assert set(found) == set(pt.MULTI_SYMBOLS) and len(found) == len(pt.MULTI_SYMBOLS) == 5
    assert found == {name: ("int", count) for name, count in COUNTS.items()}
    lib = pt.load_library()
    for name, (ret, count) in found.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, name
        assert fn.restype is C.c_int, name


def test_multi_symbols_are_in_no_other_table():
    others = set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS) | set(pt.POST_SYMBOLS) | set(pt.STATS_SYMBOLS) | set(pt.ADAPTIVE_SYMBOLS)
    assert not set(pt.MULTI_SYMBOLS) & others
    assert len(set(pt.MULTI_SYMBOLS)) == len(pt.MULTI_SYMBOLS)
    # the five existing tables keep their sizes
    assert (len(pt.ABI_SYMBOLS) + len(pt.DEBUG_SYMBOLS), len(pt.POST_SYMBOLS), len(pt.STATS_SYMBOLS), len(pt.ADAPTIVE_SYMBOLS)) == (48, 4, 5, 4)


def test_multi_info_matches_the_header():
    text = open(os.path.join(ROOT, "include", "ptr_multi.h")).read()
    assert int(re.search(r"#define PTR_MULTI_MAX_PARTS (\d+)", text).group(1)) == pt.MULTI_MAX_PARTS == 64
    assert C.sizeof(pt.PtrMultiInfo) == 8 + 3 * 8 * 64
    assert [name for name, _ in pt.PtrMultiInfo._fields_] == ["parts", "stagedParts", "partSamples", "partRenderSeconds", "partWaitSeconds"]


# --------------------------------------------------------------------------- bad arguments
def _params(min_spp=4, max_spp=16, step=4, threshold=0.1):
    return pt.PtrAdaptiveParams(min_spp, max_spp, step, threshold)


BAD_PARAMS = [_params(min_spp=1), _params(min_spp=0), _params(min_spp=8, max_spp=7), _params(step=0), _params(threshold=-0.5),
              _params(threshold=math.nan), _params(threshold=math.inf)]
W, H = 8, 8


class Buffers:
    def __init__(self):
        self.rgb = np.full((H, W, 3), 7.0, np.float32)
        self.cov = np.full((H, W, 6), 7.0, np.float32)
        self.count = np.full((H, W), 7, np.uint32)
        self.albedo = np.full((H, W, 4), 7.0, np.float32)
        self.normal = np.full((H, W, 4), 7.0, np.float32)
        self.samples = np.ones((16, H, W, 4), np.float32)

    def untouched(self):
        return all((a == 7).all() for a in (self.rgb, self.cov, self.count, self.albedo, self.normal))


def _call(name, buf, desc="ok", settings="ok", params="ok", spp=4, ids=(0, 0), n_devices=1, rgb="ok", samples="ok", size=(W, H)):
    """One call of `name` with good arguments except the ones overridden: None for a null pointer, or another value."""
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    d = C.byref(pt.PtrSceneDesc()) if desc == "ok" else desc          # never looked into by a refused call
    if settings == "ok":
        settings = pt.PtrSettings()
        settings.width, settings.height, settings.maxDepth = size[0], size[1], 2
    s = None if settings is None else C.byref(settings)
    if params == "ok":
        params = _params()
    p = None if params is None else C.byref(params)
    idl = None if ids is None else (C.c_int * max(len(ids), 1))(*ids)
    n = 0 if ids is None else len(ids)
    out = None if rgb is None else fp(buf.rgb)
    stats, info, multi = pt.PtrRenderStats(), pt.PtrAdaptiveInfo(), pt.PtrMultiInfo()
    tail = (C.byref(stats), C.byref(multi), err, len(err))
    atail = (C.byref(stats), C.byref(info), C.byref(multi), err, len(err))
    if name == "ptr_render_multi":
        rc = lib.ptr_render_multi(d, s, spp, n_devices, 0, out, C.byref(stats), err, len(err))
    elif name == "ptr_debug_render_multi_on":
        rc = lib.ptr_debug_render_multi_on(d, s, spp, idl, n, out, C.byref(stats), err, len(err))
    elif name == "ptr_render_multi_cov":
        rc = lib.ptr_render_multi_cov(d, s, spp, n_devices, 0, out, fp(buf.cov), fp(buf.albedo), fp(buf.normal), *tail)
    elif name == "ptr_multi_debug_cov_on":
        rc = lib.ptr_multi_debug_cov_on(d, s, spp, idl, n, out, fp(buf.cov), fp(buf.albedo), fp(buf.normal), *tail)
    elif name == "ptr_render_multi_adaptive":
        rc = lib.ptr_render_multi_adaptive(d, s, p, n_devices, 0, out, fp(buf.cov), up(buf.count), fp(buf.albedo), fp(buf.normal), *atail)
    elif name == "ptr_multi_debug_adaptive_on":
        rc = lib.ptr_multi_debug_adaptive_on(d, s, p, idl, n, out, fp(buf.cov), up(buf.count), fp(buf.albedo), fp(buf.normal), *atail)
    else:
        smp = None if samples is None else fp(buf.samples)
        rc = lib.ptr_multi_debug_adaptive_frame(size[0], size[1], p, smp, idl, n, out, fp(buf.cov), up(buf.count), C.byref(info), err, len(err))
    return rc, err.value.decode()


def _bad_cases(name):
    cases = [dict(rgb=None), dict(size=(0, H)), dict(size=(W, 0))]
    if name != "ptr_multi_debug_adaptive_frame":
        cases += [dict(desc=None), dict(settings=None)]
    else:
        cases += [dict(samples=None)]
    if "adaptive" in name:
        cases += [dict(params=None)] + [dict(params=p) for p in BAD_PARAMS]
    elif name not in PLAIN:
        cases += [dict(spp=0), dict(spp=1)]                      # a sample covariance needs two samples
    if "debug" in name:
        cases += [dict(ids=None), dict(ids=()), dict(ids=(0,) * 65)]
    else:
        cases += [dict(n_devices=65)]
    return cases


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_bad_arguments_are_refused_by_name(name):
    buf = Buffers()
    for case in _bad_cases(name):
        rc, message = _call(name, buf, **case)
        assert rc == 1 and message.startswith(name + ":"), (case, rc, message)
    if "adaptive" in name:
        assert "minSpp" in _call(name, buf, params=_params(min_spp=1))[1]
        assert "threshold" in _call(name, buf, params=_params(threshold=math.nan))[1]
    assert buf.untouched()


@pytest.mark.parametrize("name", PLAIN)
def test_plain_frame_refuses_bad_arguments_by_name(name):
    buf = Buffers()
    cases = _bad_cases(name)
    assert len(cases) == (8 if "debug" in name else 6)       # three null pointers, two sizes, the device count or the three id lists
    for case in cases:
        rc, message = _call(name, buf, **case)
        assert rc == 1 and message.startswith(name + ":"), (case, rc, message)
    assert buf.untouched()


@pytest.mark.parametrize("name", PLAIN)
def test_plain_frame_takes_any_spp_and_fails_loudly_without_gpu(name):
    """spp = 0 and spp = 1 are no refusal of the plain frame's: without a GPU such a call gets as far as the device check."""
    if pt.device_count() > 0:
        pytest.skip("a GPU is present")
    buf = Buffers()
    for spp in (4, 1, 0):
        rc, message = _call(name, buf, spp=spp)
        assert rc == 2 and message == name + ": no HIP device (the HIP path has no CPU fallback)", (spp, rc, message)
    assert buf.untouched()


def test_multi_fails_loudly_without_gpu():
    if pt.device_count() > 0:
        pytest.skip("a GPU is present")
    buf = Buffers()
    for name in COUNTS:
        rc, message = _call(name, buf)
        assert rc == 2 and message.startswith(name + ":") and "no CPU fallback" in message, (name, rc, message)
    assert buf.untouched()
    host = pt.HostScene.load(os.path.join(ROOT, "tests", "golden", "smoke.scene"))
    s = host.settings_for(width=8, height=8)
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.render_multi_adaptive(host.desc, s, _params())
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.render_multi_cov(host.desc, s, 4, device_ids=[0, 0])
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.multi_adaptive_debug_frame(np.ones((16, 8, 8, 3), np.float32), _params(), [0])


# --------------------------------------------------------------------------- the inputs discriminate
CASES = [(67, 45, 12), (130, 70, 16)]           # width, height, maxSpp (min 4, step 4)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%dx%d" % c[:2])
def synthetic(request):
    w, h, max_spp = request.param
    x = adaptive_ref.synthetic_samples(max_spp, h, w)
    p = adaptive_ref.params(4, max_spp, 4, multi_ref.median_threshold(x, 4, 4))
    return w, h, x, p, adaptive_ref.adaptive_ref(x, p)


def test_first_lists_partition_the_image():
    for w, h, parts in ((67, 45, 3), (11, 9, 2), (5, 3, 1), (130, 70, 9)):
        lists = [multi_ref.partition_pixels(w, h, q, parts) for q in range(parts)]
        assert sorted(np.concatenate(lists)) == list(range(w * h))
        for q, l in enumerate(lists):
            assert ((l // w // 8) % parts == q).all()
    assert np.array_equal(multi_ref.partition_pixels(11, 9, 0, 1), adaptive_ref.pixel_order(11, 9))


def test_true_halo_is_the_single_device_restatement(synthetic):
    w, h, x, p, want = synthetic
    for parts in (1, 2, 3, multi_ref.band_count(h)):
        got = multi_ref.multi_ref(x, p, parts)
        assert np.array_equal(got.count, want.count), parts
        assert np.array_equal(got.rgb, want.rgb, equal_nan=True) and np.array_equal(got.cov, want.cov, equal_nan=True), parts
        assert got.rounds == want.rounds and got.active_after == want.active_after, parts
        assert sum(got.part_samples) == int(want.count.sum())


def test_a_missing_or_stale_halo_changes_the_frame(synthetic):
    """What makes GPU test 1 a test of the exchange: on these inputs a protocol without the halo, or with the halo of round 0 only, ends
    with other counts in at least 20 pixels, for every P >= 2."""
    w, h, x, p, want = synthetic
    for parts in (2, 3, multi_ref.band_count(h)):
        for halo in ("none", "stale"):
            got = multi_ref.multi_ref(x, p, parts, halo=halo)
            changed = int((got.count != want.count).sum())
            print("%dx%d P=%d halo %s: %d pixels end with another count" % (w, h, parts, halo, changed))
            assert changed >= 20, (parts, halo, changed)


# --------------------------------------------------------------------------- the barrier
def test_round_barrier_program(tmp_path):
    """tools/round_barrier_check.cpp: 1, 2 and 9 threads through 1,000 rounds of two barriers, then every thread in turn failing instead
    of arriving.  A barrier that hangs on the missing thread is a failure by the time limit."""
    exe = str(tmp_path / "round_barrier_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I" + os.path.join(ROOT, "metal-pathtracer-arm64_amd", "csrc", "host"),
                            os.path.join(ROOT, "tools", "round_barrier_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run(["timeout", "-k", "2", "20", exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "0 finding(s) in all" in run.stdout
