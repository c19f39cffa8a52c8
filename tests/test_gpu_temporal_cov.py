"""Temporal accumulation that carries covariance, on the device (include/ptr_temporal_cov.h): k_temporal_accumulate_cov against the numpy
restatement (tests/temporal_cov_ref.py) and against k_temporal_accumulate, and whole steps on static, moving and relit scenes.  Every
comparison is exact (array_equal, NaN-aware) unless it says otherwise."""
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import ctypes as C

import numpy as np
import pytest

import deform_scenes as dsc
import temporal_cases as tc
import temporal_cov_ref as cref
import temporal_ref as ref
import traversal_scenes as ts
from test_gpu_dynamic import matrix_of, rotation
from test_gpu_temporal import MISS, hosts, same, settings_of, tilted_camera, upload, words   # noqa: F401 (hosts is a fixture)

pt = ts.pt
pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("colour", "length", "history", "covariance", "covariance history")


def differing(g, x):
    return int((~((g == x) | (np.isnan(g) & np.isnan(x)))).sum())


def cov_step(temporal, s, rgb, cov, **kw):
    out = temporal.step(s, rgb, cov, **kw)
    assert out["cov"].shape == (s.height, s.width, 6) and out["cov"].dtype == F
    return out


# --------------------------------------------------------------------------------------------------------------------- 1. the kernel alone
def noisy_covariances(w, h, seed):
    """The frame's covariance and the covariance history for tc.noisy_case: diagonals over four decades, so that the consistency test
    rejects some pixels and keeps others at every rejectSigma > 0 used; small signed off-diagonals; and NaN, +inf, -inf and negative
    components in both."""
    rng = np.random.default_rng(seed)

    def one():
        c = np.zeros((h, w, 6), F)
        c[..., :3] = (10.0 ** rng.uniform(-4.0, 0.0, (h, w, 1)) * rng.uniform(0.5, 1.0, (h, w, 3))).astype(F)
        c[..., 3:] = (c[..., :3].min(axis=2, keepdims=True) * rng.uniform(-0.5, 0.5, (h, w, 3))).astype(F)
        bad = rng.random((h, w, 6))
        c[bad < 0.01] = np.nan
        c[(bad >= 0.01) & (bad < 0.02)] = np.inf
        c[(bad >= 0.02) & (bad < 0.03)] = -np.inf
        c[(bad >= 0.03) & (bad < 0.05)] *= F(-1)
        return c
    return one(), one()


@pytest.mark.parametrize("size", [(1, 1), (67, 45), (257, 3)], ids=lambda s: "%dx%d" % s)
def test_accumulate_cov_kernel_equals_the_reference_and_the_plain_kernel(size):
    w, h = size
    cams = (tilted_camera(w, h, (0.1, -0.2, 0.3), 0.05), tilted_camera(w, h, (-0.05, 0.1, 0.2), -0.03))
    behind = tilted_camera(w, h, (0.0, 0.0, -3.0), 0.0)
    cases = [("zero", (0.0, 0.0), cams[0], cams[0], 32), ("integer", (3.0, -2.0), cams[0], cams[0], 32),
             ("integer, maxHistory 1", (3.0, -2.0), cams[0], cams[0], 1), ("fractional", (0.37, 1.62), cams[0], cams[1], 3),
             ("off-image", (w + 5.0, 0.0), cams[0], cams[1], 32), ("two cameras", (-1.25, 0.5), cams[1], cams[0], 32),
             ("behind the camera", (0.0, 0.0), cams[0], cams[0], 32)]
    rejected_somewhere = kept_somewhere = 0
    for k, (name, motion, cam_cur, cam_prev, max_history) in enumerate(cases):
        rgb, cur, prev, history = tc.noisy_case(w, h, 10 * k + w, motion, cam_cur, cam_prev)
        cov, cov_history = noisy_covariances(w, h, 1000 + 10 * k + w)
        if name == "zero":
            cur[2][..., :3] = cur[0][..., :3]
        if name == "behind the camera":
            cam_prev = behind
        p = pt.PtrTemporalParams.defaults(maxHistory=max_history)
        plain = pt.debug_temporal_accumulate(rgb, cur, prev, history, cam_cur, cam_prev, p, True)
        for sigma, has_history in ((0.0, True), (0.5, True), (3.0, True), (3.0, False)):
            cp = pt.PtrTemporalCovParams.defaults(rejectSigma=sigma)
            got = pt.debug_temporal_accumulate_cov(rgb, cov, cur, prev, history, cov_history, cam_cur, cam_prev, p, cp, has_history)
            want = cref.accumulate_cov(rgb, cov, cur, prev, history, cov_history, cam_cur, cam_prev, max_history=max_history,
                                       reject_sigma=sigma, has_history=has_history)
            for g, x, what in zip(got, want, NAMES):
                assert g.shape == x.shape and same(g, x), "%s, %s, sigma %g, history %s: %s differs on %d values" % (
                    size, name, sigma, has_history, what, differing(g, x))
            assert np.isfinite(want[3]).all(), "no covariance leaves the filter that is not finite"
            hit = (words(cur[2]) != MISS) & np.isfinite(rgb).all(axis=2)
            assert (want[3][~hit] == 0).all()
            if not has_history:
                assert same(want[3][hit], np.where(np.isfinite(cov), cov, F(0))[hit])
            elif sigma == 0.0:   # which taps count is unchanged: the plain kernel's colour, length and colour history, bit for bit
                for g, x, what in zip(got[:3], plain, NAMES):
                    assert same(g, x), "%s, %s: %s differs from k_temporal_accumulate on %d values" % (size, name, what, differing(g, x))
                blends = plain[1] > 1
            else:
                rejected_somewhere += int((blends & (want[1] == 1)).sum())
                kept_somewhere += int((blends & (want[1] > 1)).sum())
    if w > 1:   # the cases are what they say: the consistency test both rejects and keeps
        assert rejected_somewhere > 0 and kept_somewhere > 0, (rejected_somewhere, kept_somewhere)


# --------------------------------------------------------------------------------------------------------------------- 2. a static sequence
def test_static_sequence_carries_the_covariance_of_the_running_mean(hosts):
    """Scene A at 67x45, six frames of 2 spp with a seed each (test_static_sequence_is_the_running_mean's sequence, with the frames'
    covariances).  Every output of every step equals the restatement fed the downloaded records and its own previous outputs, at the
    default rejectSigma; with rejectSigma 0 colour and length are a plain handle's bit for bit, and on the pixels whose own tap counts
    in every frame out_cov is (sum of the frames' covariances) / k^2 within rtol 1e-5 (test_temporal_cov_host.py says why 1e-5).

    The 1e-5 is taken of (sum of the magnitudes of the frames' values) / k^2.  Where the k values share a sign - every variance, and most
    covariances - that IS the sum, and the check is rtol 1e-5 on it to the letter.  An off-diagonal value changes sign between frames
    at a few pixels, the terms cancel, and the recurrence's roundings, which are relative to its terms, are no longer small beside what
    is left of the sum: against the bare sum these few values were off by up to 2.1e-5 (frame 3), which no float32 evaluation of the
    recurrence can avoid; the simulation behind the bound drew its covariances positive.  Measured over the six frames: 3.2e-7 at most
    where the values share a sign (86 to 95 % of them, every variance among them), 3.2e-7 at most relative to the sum of magnitudes."""
    host = hosts("A")
    dev = upload(host)
    try:
        w, h = 67, 45
        p = pt.PtrTemporalParams.defaults()
        testing, summing, plain = dev.temporal(w, h, cov=True), dev.temporal(w, h, cov=pt.PtrTemporalCovParams.defaults(rejectSigma=0.0)), dev.temporal(w, h)
        assert testing.carries_cov and summing.carries_cov and not plain.carries_cov
        cam = pt.debug_temporal_camera(settings_of(host, w, h))
        frames, covs, recs = [], [], []
        want = None
        steady = never = None
        for k in range(6):
            s = settings_of(host, w, h, seed=500 + k)
            rgb, cov, _ = dev.render_image_cov(s, 2)
            frames.append(rgb)
            covs.append(cov)
            out = cov_step(testing, s, rgb, cov)
            recs.append(testing.records())
            want = cref.accumulate_cov(rgb, cov, recs[k], recs[k - 1][:2] if k else recs[k][:2], want[2] if k else np.zeros((h, w, 4), F),
                                       want[4] if k else np.zeros((h, w, 6), F), cam, cam, has_history=k > 0)
            for key, x in zip(("rgb", "length", "cov"), (want[0], want[1], want[3])):
                assert same(out[key], x), "frame %d, %s: %d values differ from the reference" % (k, key, differing(out[key], x))
            out0, out_plain = cov_step(summing, s, rgb, cov), plain.step(s, rgb)
            assert same(out0["rgb"], out_plain["rgb"]) and np.array_equal(out0["length"], out_plain["length"]), k
            (r0, r1, r2) = recs[k]
            hit = (words(r2) != MISS) & np.isfinite(rgb).all(axis=2)
            if k == 0:
                steady, never = hit.copy(), ~hit
                assert same(out0["cov"][hit], np.where(np.isfinite(cov), cov, F(0))[hit]) and (out0["cov"][~hit] == 0).all()
                continue
            q0, q1, _ = recs[k - 1]
            to_camera = r2[..., :3] - cam[0]
            counts = hit & (words(q0) == words(r0)) & (ref.dot(q1[..., :3], r1[..., :3]) >= F(p.normalCos)) & \
                (np.abs(ref.dot(r2[..., :3] - q0[..., :3], q1[..., :3])) <= F(p.planeTolerance) * np.sqrt(ref.dot(to_camera, to_camera)))
            steady &= counts
            never &= ~hit
            stack = np.asarray(covs, np.float64)[:, steady]
            exact, scale = stack.sum(axis=0) / ((k + 1) ** 2), np.abs(stack).sum(axis=0) / ((k + 1) ** 2)
            got = out0["cov"][steady].astype(np.float64)
            one_sign = scale == np.abs(exact)
            with np.errstate(all="ignore"):
                literal = np.where(exact != 0, np.abs(got / exact - 1), 0)
                scaled = np.where(scale != 0, np.abs(got - exact) / scale, 0)
            print("frame %d: steady %.3f of the image; worst error of out_cov relative to the sum %.3g (%.3g where the frames' values share a "
                  "sign, %.1f %% of the values), relative to the sum of magnitudes %.3g" % (
                      k, steady.mean(), literal.max(), literal[one_sign].max(), 100.0 * one_sign.mean(), scaled.max()))
            assert (out0["length"][steady] == k + 1).all()
            assert one_sign[:, :3].all(), "variances do not change sign"
            assert (np.abs(got - exact) <= 1e-5 * scale).all(), (k, float(scaled.max()))
            assert (out0["cov"][never] == 0).all()
        assert float((steady | never).mean()) >= 0.8
        for t in (testing, summing, plain):
            t.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 3. whole steps with motion
@pytest.mark.parametrize("motion", ["mesh", "yaw"])
def test_cov_steps_equal_the_reference_fed_the_records(hosts, motion):
    host = hosts("lit")
    dev = upload(host, dynamic=True)
    try:
        temporal = dev.temporal(48, 32, pt.PtrTemporalParams.defaults(maxHistory=2), cov=True)
        history, cov_history, prev, cam_prev = np.zeros((32, 48, 4), F), np.zeros((32, 48, 6), F), None, None
        blended = 0
        for k in range(3):
            s = settings_of(host, seed=40 + k)
            if motion == "mesh" and k:
                turn = rotation((0.0, 1.0, 0.0), np.radians(8.0 * k))
                dev.set_mesh_transforms({0: (matrix_of(host, 0).astype(np.float64) @ turn).astype(F)})
            elif motion == "yaw":
                s.cameraYaw += float(np.radians(1.0) * k)
            rgb, cov, _ = dev.render_image_cov(s, 2)
            out = cov_step(temporal, s, rgb, cov)
            records = temporal.records()
            cam = pt.debug_temporal_camera(s)
            want = cref.accumulate_cov(rgb, cov, records, prev if k else records[:2], history, cov_history, cam, cam_prev if k else cam,
                                       max_history=2, has_history=k > 0)
            for key, x in zip(("rgb", "length", "cov"), (want[0], want[1], want[3])):
                assert same(out[key], x), "%s, frame %d, %s: %d values differ from the reference" % (motion, k, key, differing(out[key], x))
            blended += int((want[1] == 2).sum()) if k else 0
            if k:
                hit = want[1] > 0
                shift = np.abs(ref.project(cam_prev, records[2][..., :3], 48, 32)[0] - ref.project(cam, records[0][..., :3], 48, 32)[0])
                assert shift[hit].max() > 0.1, "the image moved"
            history, cov_history, prev, cam_prev = want[2], want[4], records[:2], cam
        assert blended > 0, "and some of it found a history the frame agrees with"
        temporal.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 4. a moved light
def test_a_moved_light_resets_what_it_relit(hosts):
    """The `slide` scene at 48x32 and 64 spp: two frames, then the light rectangle is moved 8 units along x by set_rects, then two more.
    With rejectSigma 3 and with 0 every step equals the restatement.  No geometry in view changed, so with rejectSigma 0 every hit pixel
    keeps its history; with rejectSigma 3 the restatement itself, fed the same frames, resets in the frame after the move hit pixels
    that the rejectSigma 0 run blends: 1169 of the 1497 it blends, where at least one is asked for.  That is a choice of input checked
    against the reference, not against the kernel."""
    host = hosts("slide")
    w, h = 48, 32
    lengths = {}
    for sigma in (3.0, 0.0):
        dev = upload(host, dynamic=True)
        try:
            temporal = dev.temporal(w, h, cov=pt.PtrTemporalCovParams.defaults(rejectSigma=sigma))
            want, prev = None, None
            for k in range(4):
                if k == 2:
                    light = dsc.rect_of(host, 2)
                    light["corner"] = light["corner"] + np.array([8.0, 0.0, 0.0], F)
                    dev.set_rects({2: light})
                s = settings_of(host, w, h, seed=900 + k)
                rgb, cov, _ = dev.render_image_cov(s, 64)
                out = cov_step(temporal, s, rgb, cov)
                records = temporal.records()
                cam = pt.debug_temporal_camera(s)
                want = cref.accumulate_cov(rgb, cov, records, prev if k else records[:2], want[2] if k else np.zeros((h, w, 4), F),
                                           want[4] if k else np.zeros((h, w, 6), F), cam, cam, reject_sigma=sigma, has_history=k > 0)
                for key, x in zip(("rgb", "length", "cov"), (want[0], want[1], want[3])):
                    assert same(out[key], x), "sigma %g, frame %d, %s: %d values differ from the reference" % (sigma, k, key, differing(out[key], x))
                prev = records[:2]
                if k == 2:
                    lengths[sigma] = want[1]
            temporal.close()
        finally:
            dev.close()
    relit = (lengths[3.0] == 1) & (lengths[0.0] > 1)
    print("hit pixels reset by the consistency test in the frame after the move: %d of %d blended without it" % (relit.sum(), (lengths[0.0] > 1).sum()))
    assert relit.sum() >= 1


# --------------------------------------------------------------------------------------------------------------------- 5. host and device entry points
def test_host_and_device_cov_steps_agree(hosts):
    host = hosts("lit")
    dev = upload(host)
    try:
        s = settings_of(host)
        h, w = s.height, s.width
        on_host, out_of_place, in_place = (dev.temporal(w, h, cov=True) for _ in range(3))
        zeros = lambda c: torch.zeros((h, w, c), dtype=torch.float32, device="cuda:0")
        for k in range(3):
            s.seed = 70 + k
            rgb, cov, _ = dev.render_image_cov(s, 2)
            want = cov_step(on_host, s, rgb, cov, want_aovs=True)
            d_rgb, d_cov = torch.from_numpy(rgb).cuda(), torch.from_numpy(cov).cuda()
            outs = {name: zeros(c) for name, c in (("rgb", 3), ("cov", 6), ("length", 1), ("albedo", 4), ("normal", 4))}
            info = out_of_place.step_device(s, d_rgb, outs["rgb"], outs["length"], outs["albedo"], outs["normal"], want_info=True, cov=d_cov,
                                            out_cov=outs["cov"])
            assert info["frameIndex"] == k and info["surfaceMs"] > 0 and info["accumulateMs"] > 0
            torch.cuda.synchronize()
            assert same(d_rgb.cpu().numpy(), rgb) and same(d_cov.cpu().numpy(), cov), "out of place: the inputs are left alone"
            for name in outs:
                assert same(outs[name].cpu().numpy().reshape(want[name].shape), want[name]), (k, name)
            # in place: d_out_rgb == d_rgb and d_out_cov == d_cov, on torch's current stream
            assert in_place.step_device(s, d_rgb, cov=d_cov) is None
            torch.cuda.synchronize()
            assert same(d_rgb.cpu().numpy(), want["rgb"]) and same(d_cov.cpu().numpy(), want["cov"]), k
            # the layout contract: out_cov goes as it is into the denoiser
            pt.denoise_device(outs["rgb"].data_ptr(), outs["albedo"].data_ptr(), outs["normal"].data_ptr(), w, h,
                              stream=torch.cuda.current_stream(0).cuda_stream, d_cov=outs["cov"].data_ptr())
            torch.cuda.synchronize()
            assert same(outs["rgb"].cpu().numpy(), pt.denoise(want["rgb"], want["albedo"], want["normal"], cov=want["cov"])), k
        for t in (on_host, out_of_place, in_place):
            t.close()
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 6. reset and refusals
def test_reset_and_refusals_leave_both_histories_alone(hosts):
    host = hosts("pair")
    dev = upload(host)
    try:
        s = settings_of(host)
        h, w = s.height, s.width
        rng = np.random.default_rng(3)
        frames = rng.random((3, h, w, 3)).astype(F)
        covs = (rng.random((3, h, w, 6)) * 0.5).astype(F)   # (wide enough that the default rejectSigma keeps most of the random frames)
        twin, refused, plain = dev.temporal(w, h, cov=True), dev.temporal(w, h, cov=True), dev.temporal(w, h)
        want = [cov_step(twin, s, f, c) for f, c in zip(frames[:2], covs[:2])]
        assert want[1]["info"]["hadHistory"] == 1 and (want[1]["length"] == 2).any()
        first = cov_step(refused, s, frames[0], covs[0])
        assert same(first["rgb"], want[0]["rgb"]) and same(first["cov"], want[0]["cov"])
        lib = pt.load_library()
        err = C.create_string_buffer(256)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        out, out_cov = np.zeros_like(frames[0]), np.zeros_like(covs[0])
        n = h * w
        d_rgb, d_cov = torch.from_numpy(frames[1]).cuda(), torch.from_numpy(covs[1]).cuda()
        vp = lambda t, offset=0: C.c_void_p(t.data_ptr() + offset)
        step_device = lambda *ptrs: lib.ptr_temporal_step_cov_device(refused._h, C.byref(s), *ptrs, None, None, None, None, None, err, len(err))
        # a host pointer for d_cov
        assert step_device(vp(d_rgb), C.c_void_p(covs[1].ctypes.data), vp(d_rgb), vp(d_cov)) == 1
        assert err.value.startswith(b"ptr_temporal_step_cov_device: d_cov is") and b"not" in err.value
        # an unaligned buffer (8 B for the covariances) and a short one
        big = torch.zeros(n * 6 + 8, dtype=torch.float32, device="cuda:0")
        assert step_device(vp(d_rgb), vp(big, 4), vp(d_rgb), vp(d_cov)) == 1 and err.value == b"ptr_temporal_step_cov_device: d_cov is not 8 B aligned"
        assert step_device(vp(d_rgb), vp(d_cov), vp(d_rgb), vp(big, 4)) == 1 and err.value == b"ptr_temporal_step_cov_device: d_out_cov is not 8 B aligned"
        # (torch hands out pieces of larger allocations, and the library knows the allocation's end, not the tensor's: the short buffer is
        # the last n * 24 - 8 bytes of the allocation `big` lies in.  Its partner, 16 B lower, is long enough and overlaps it at an offset,
        # so the call is refused whatever the length check says, and the message says which check spoke)
        segment = next(g for g in torch.cuda.memory_snapshot() if g["address"] <= big.data_ptr() < g["address"] + g["total_size"])
        end = segment["address"] + segment["total_size"]
        short, fits = C.c_void_p(end - (n * 24 - 8)), C.c_void_p(end - (n * 24 + 8))
        assert step_device(vp(d_rgb), fits, vp(d_rgb), short) == 1 and err.value == b"ptr_temporal_step_cov_device: d_out_cov is shorter than the image"
        assert step_device(vp(d_rgb), short, vp(d_rgb), fits) == 1 and err.value == b"ptr_temporal_step_cov_device: d_cov is shorter than the image"
        # d_cov overlapping d_out_cov at an offset
        assert step_device(vp(d_rgb), vp(big), vp(d_rgb), vp(big, 32)) == 1 and b"d_cov and d_out_cov overlap" in err.value
        with pytest.raises(pt.PtrError, match="d_cov and d_out_cov overlap"):
            refused.step_device(s, d_rgb, cov=big[:n * 6], out_cov=big[8:n * 6 + 8])
        # settings of another size
        other = settings_of(host, w + 1, h)
        assert lib.ptr_temporal_step_cov(refused._h, C.byref(other), fp(frames[1]), fp(covs[1]), fp(out), fp(out_cov), None, None, None, None, err, len(err)) == 1
        assert err.value.startswith(b"ptr_temporal_step_cov: the settings are 49x32")
        # a null cov, a null out_cov
        assert lib.ptr_temporal_step_cov(refused._h, C.byref(s), fp(frames[1]), None, fp(out), fp(out_cov), None, None, None, None, err, len(err)) == 1
        assert err.value == b"ptr_temporal_step_cov: null argument"
        assert step_device(vp(d_rgb), None, vp(d_rgb), vp(d_cov)) == 1 and err.value == b"ptr_temporal_step_cov_device: null argument"
        assert step_device(vp(d_rgb), vp(d_cov), vp(d_rgb), None) == 1 and err.value == b"ptr_temporal_step_cov_device: null argument"
        # a handle is one kind for life
        with pytest.raises(pt.PtrError, match="ptr_temporal_step: this handle carries covariance"):
            refused.step(s, frames[1])
        with pytest.raises(pt.PtrError, match="ptr_temporal_step_device: this handle carries covariance"):
            refused.step_device(s, d_rgb)
        with pytest.raises(pt.PtrError, match="ptr_temporal_step_cov: this handle carries no covariance"):
            plain.step(s, frames[1], covs[1])
        with pytest.raises(pt.PtrError, match="ptr_temporal_step_cov_device: this handle carries no covariance"):
            plain.step_device(s, d_rgb, cov=d_cov)
        with pytest.raises(pt.PtrError, match="rejectSigma"):
            dev.temporal(w, h, cov=pt.PtrTemporalCovParams.defaults(rejectSigma=-1.0))
        with pytest.raises(pt.PtrError, match="maxHistory"):
            dev.temporal(w, h, pt.PtrTemporalParams.defaults(maxHistory=0), cov=True)
        with pytest.raises(pt.PtrError, match="not a torch tensor"):
            refused.step_device(s, d_rgb, cov=covs[1])
        with pytest.raises(pt.PtrError, match="contiguous float32"):
            refused.step_device(s, d_rgb, cov=torch.zeros((h, w, 3), device="cuda:0"))
        torch.cuda.synchronize()
        assert same(d_rgb.cpu().numpy(), frames[1]) and same(d_cov.cpu().numpy(), covs[1]), "a refused call writes nothing"
        # after all of them: the step of the twin that never saw a refused call
        got = cov_step(refused, s, frames[1], covs[1])
        assert got["info"]["frameIndex"] == 1 and np.array_equal(got["length"], want[1]["length"])
        assert same(got["rgb"], want[1]["rgb"]) and same(got["cov"], want[1]["cov"])
        # ... and the plain handle still is a plain handle
        assert same(plain.step(s, frames[0])["rgb"], frames[0])
        # reset: the next step is a first step, out_cov = Cc
        refused.reset()
        again = cov_step(refused, s, frames[2], covs[2])
        assert again["info"]["hadHistory"] == 0 and again["info"]["frameIndex"] == 0 and np.array_equal(again["rgb"], frames[2])
        hit = again["length"] == 1
        assert hit.any() and np.array_equal(again["cov"][hit], covs[2][hit]) and (again["cov"][~hit] == 0).all()
        for t in (twin, refused, plain):
            t.close()
        with pytest.raises(pt.PtrError, match="closed"):
            refused.step(s, frames[0], covs[0])
    finally:
        dev.close()
