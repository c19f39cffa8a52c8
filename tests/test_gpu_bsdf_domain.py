"""evalBsdf / sampleBsdf on the device (the probes debug_eval_bsdf, debug_sample_bsdf, debug_sample_lobes) against the oracle over every
class of bsdf_domain.py: tilted and downward normals, both branches of makeFrame, grazing and below-surface wo, wi in both hemispheres,
at the mirror direction, equal and opposite to wo and inside the lobe, materials on either side of every threshold, six modes.

Equal to the oracle everywhere: the random state afterwards, isDelta, the rows evaluation zeroes for a side test.  The device's own
outputs are finite, non-negative and unit as the oracle's are (test_bsdf_domain_host.py).  A (material, class) pair that the oracle itself
carries across the suite's tolerance under a one-ulp move of wo in at most CAP / 2 of its rows (bsdf_domain.ILL_CONDITIONED lists the
others) is held to those tolerances in 1 - CAP of its rows; the others to directions within 3e-4 and to test_gpu_parity's loose bound
for narrow lobes in 99 % of their rows.  Sample against evaluate is asked of the device's own pair of outputs, within four times the
oracle's figure (ORACLE_MEASURED): both sides see one direction, so the bound is as tight as the oracle's own figure; the factor covers
ocml against glibc in sin / cos / sqrt, compounded through D.  For the group metal_narrow that figure is 2.8e8 to 5.2e11, and four times
it checks nothing: at alpha^2 <= 1.6e-7 the oracle's own sampler and evaluation disagree without limit (it samples weights of 3.7e8 at
a pdf of 1e-8 for roughness 1.1e-3: ggxD is a2 / 0 or rounding noise there).  The group stays in the list because the issue
sets it; what holds it is the comparison with the oracle above.  No bound here was taken from the device's output.

The narrow metals (roughness 1.1e-3 and 0.02) under the VNDF sampler are why sampleGgxVndf takes its sine and cosine in double: with
ocml's sinf / cosf 1.0 to 5.8 % of their rows lay past the loose bound (1 % is allowed) and two sample-against-evaluate weights reached
1.8e9 against a bound of 1.12e9, because ggxD at alpha^2 <= 1.6e-7 turns the last bit of the half vector into another value of D.  With
the rounded-once pair the worst class leaves 14 of 4096 rows past the loose bound and the largest identity figure is a quarter of its
bound.
"""
import numpy as np
import pytest

import bsdf_domain as bd
import oracle_lib as ol
import test_bsdf_domain_host as dh

pt = bd.pt
pytestmark = pytest.mark.gpu

DIR_ATOL = 3e-4   # directions of ill-conditioned pairs (test_gpu_parity.test_metal_pbr_semantics)


def _group(group):
    return [(name, m) for name, g, m in bd.materials() if g == group]


def _worst(a, b):
    """Largest |a - b| relative to |b| + 1e-2 (test_gpu_parity._rel)."""
    return float((np.abs(a.astype(np.float64) - b) / (np.abs(b.astype(np.float64)) + 1e-2)).max(initial=0.0))


def _tally(tally, cls, rows, capped, well=0.0, ill=0.0):
    """Per class: rows compared, rows under the caps, largest difference (_worst) among the agreeing rows of well-conditioned pairs (held
    to the suite's tolerance) and of ill-conditioned ones (held to the loose one)."""
    old = tally.get(cls, (0, 0, 0.0, 0.0))
    tally[cls] = (old[0] + rows, old[1] + capped, float("%.2g" % max(old[2], well)), float("%.2g" % max(old[3], ill)))


@pytest.mark.parametrize("group", bd.GROUPS)
def test_sample_bsdf_over_the_domain(group):
    """Every sample class of every material of the group, in every mode it runs in; every class that misses is named."""
    inp, front, states, where = bd.sample_batch()
    rows = capped = 0
    worst, failed, tally = {}, [], {}
    for name, m in _group(group):
        for mode in bd.modes_of(group):
            s = bd.settings(mode)
            lobes, g, gs, _ = pt.debug_sample_lobes(m, s, inp, front, states)
            g2, gs2 = pt.debug_sample_bsdf(m, s, inp, front, states)
            o, os_ = ol.sample_bsdf(m, s, inp, front, states)
            what = "%s, %s" % (name, mode)
            assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and np.array_equal(gs, gs2), what   # one function behind both probes
            assert np.array_equal(gs, os_), (what, int((gs != os_).sum()))
            assert np.array_equal(g[:, 7], o[:, 7]) and np.array_equal(lobes[:, 2], g[:, 7]), what
            ev = None
            if (group, mode) in bd.IDENTITY:
                ev = pt.debug_eval_bsdf(m, s, np.concatenate([inp, g[:, 0:3]], axis=1))
            for cls, at in where.items():
                what = "%s, %s, sample %s" % (name, mode, cls)
                gc, oc = g[at], o[at]
                dh.check_sample_outputs(gc, gs[at], m, what)
                agree = (gc[:, 6] > 0) == (oc[:, 6] > 0)
                both = agree & (oc[:, 6] > 0)
                rows += len(gc)
                if cls not in bd.ILL_CONDITIONED[name]:
                    close = np.isclose(gc[both], oc[both], **bd.SAMPLE_TOL).all(axis=1)
                    capped += int((~agree).sum() + (~close).sum())
                    _tally(tally, cls, len(gc), int((~agree).sum() + (~close).sum()), well=_worst(gc[both][close], oc[both][close]))
                    worst["well"] = max(worst.get("well", 0.0), _worst(gc[both][close], oc[both][close]))
                    if agree.mean() < 1 - bd.CAP or (~close).sum() > bd.CAP * len(gc):
                        failed.append((what, "%d rows valid on one side only, %d past the tolerance" % ((~agree).sum(), (~close).sum())))
                else:
                    loose = np.isclose(gc[both], oc[both], **bd.LOOSE_TOL).all(axis=1)
                    capped += int((~agree).sum() + (~loose).sum())
                    _tally(tally, cls, len(gc), int((~agree).sum() + (~loose).sum()), ill=_worst(gc[both][loose], oc[both][loose]))
                    d = float(np.abs(gc[both, 0:3] - oc[both, 0:3]).max(initial=0.0))
                    worst["ill direction"] = max(worst.get("ill direction", 0.0), d)
                    print("%s: ill-conditioned, %d of %d rows valid on one side only, %d past the loose bound, directions off by %.2e at most"
                          % (what, int((~agree).sum()), len(gc), int((~loose).sum()), d))
                    if agree.mean() < 0.99 or d > DIR_ATOL or (~loose).sum() > 0.01 * len(gc):
                        failed.append((what, "ill-conditioned: %d rows valid on one side only, %d past the loose bound, directions off by %.2e"
                                       % ((~agree).sum(), (~loose).sum(), d)))
                if ev is not None and cls in bd.IDENTITY_CLASSES:
                    ok = (gc[:, 6] > 0) & (gc[:, 7] == 0)
                    e_pdf, e_weight = bd.identity_errors(gc[ok], bd.expected_weight(ev[at][ok], inp[at][ok, 3:6], gc[ok, 0:3]))
                    _, b_pdf, b_weight = bd.ORACLE_MEASURED[group][cls]
                    print("%s: sample against evaluate on %d rows: pdf %.3g (bound %.3g), weight %.3g (bound %.3g)"
                          % (what, int(ok.sum()), e_pdf.max(initial=0.0), 4 * b_pdf, e_weight.max(initial=0.0), 4 * b_weight))
                    assert ok.mean() > 0.2, what
                    if not (e_pdf.max(initial=0.0) <= 4 * b_pdf and e_weight.max(initial=0.0) <= 4 * b_weight):
                        failed.append((what, "sample against evaluate: pdf %.3g (bound %.3g), weight %.3g (bound %.3g)"
                                       % (e_pdf.max(), 4 * b_pdf, e_weight.max(), 4 * b_weight)))
    print("%s: %d sample rows compared, %d under the caps, largest difference of a well-conditioned row %.2e (rtol %.0e), of an ill-conditioned "
          "direction %.2e (bound %.0e)" % (group, rows, capped, worst.get("well", 0.0), bd.SAMPLE_TOL["rtol"], worst.get("ill direction", 0.0), DIR_ATOL))
    print("%s, sample rows / rows under the caps / largest well- and ill-conditioned difference by class: %s" % (group, tally))
    assert not failed, failed   # (every class that misses, by name)


@pytest.mark.parametrize("group", bd.GROUPS)
def test_eval_bsdf_over_the_domain(group):
    rows = capped = 0
    worst, failed, tally = 0.0, [], {}
    for name, m in _group(group):
        for mode in bd.modes_of(group):
            s = bd.settings(mode)
            inp, where = bd.eval_batch(lambda i, f, st: ol.sample_bsdf(m, s, i, f, st)[0])
            g = pt.debug_eval_bsdf(m, s, inp)
            o = ol.eval_bsdf(m, s, inp)
            assert np.array_equal(g[:, 4], o[:, 4]), (name, mode)
            for cls, at in where.items():
                what = "%s, %s, eval %s" % (name, mode, cls)
                gc, oc = g[at], o[at]
                zero, sure = dh.check_eval_outputs(gc, inp[at], m, mode, what)
                ozero = ~oc[:, 0:4].any(axis=1)
                assert np.array_equal(zero, ozero), (what, int((zero != ozero).sum()))   # every row: `sure` serves the float64 rules alone
                rows += len(gc)
                ill = cls in bd.ILL_CONDITIONED[name]
                close = np.isclose(gc[:, 0:4], oc[:, 0:4], **(bd.LOOSE_TOL if ill else bd.EVAL_TOL)).all(axis=1)
                capped += int((~close).sum())
                _tally(tally, cls, len(gc), int((~close).sum()), **{"ill" if ill else "well": _worst(gc[close, 0:4], oc[close, 0:4])})
                if ill:
                    print("%s: ill-conditioned, %d of %d rows past the loose bound" % (what, int((~close).sum()), len(gc)))
                    if (~close).sum() > 0.01 * len(gc):
                        failed.append((what, "ill-conditioned: %d rows past the loose bound" % (~close).sum()))
                else:
                    worst = max(worst, _worst(gc[close, 0:4], oc[close, 0:4]))
                    if (~close).sum() > bd.CAP * len(gc):
                        failed.append((what, "%d rows past the tolerance" % (~close).sum()))
    print("%s: %d evaluation rows compared, %d under the caps, largest difference of a well-conditioned row %.2e (rtol %.0e)"
          % (group, rows, capped, worst, bd.EVAL_TOL["rtol"]))
    print("%s, evaluation rows / rows under the caps / largest well- and ill-conditioned difference by class: %s" % (group, tally))
    assert not failed, failed


def test_rows_do_not_depend_on_the_batch():
    """Rows 0, 1 and 4096 of a batch of 4097 (the last one alone in its block) equal the same rows sent alone, bit for bit."""
    inp, front, states, where = bd.sample_batch()
    at = where["band/grazing"]
    si = np.concatenate([inp[at], inp[0:1]])
    sf, ss = np.concatenate([front[at], front[0:1]]), np.concatenate([states[at], states[0:1]])
    picked = {}
    for name, group, m in bd.materials():
        picked.setdefault(group, (name, m))
    for group, (name, m) in picked.items():
        mode = bd.modes_of(group)[-2]
        s = bd.settings(mode)
        g, gs = pt.debug_sample_bsdf(m, s, si, sf, ss)
        lobes, _, _, _ = pt.debug_sample_lobes(m, s, si, sf, ss)
        ei = np.concatenate([si, np.where(g[:, 6:7] > 0, g[:, 0:3], -si[:, 6:9])], axis=1).astype(np.float32)
        e = pt.debug_eval_bsdf(m, s, ei)
        assert len(g) == 4097
        for r in (0, 1, 4096):
            g1, gs1 = pt.debug_sample_bsdf(m, s, si[r:r + 1], sf[r:r + 1], ss[r:r + 1])
            l1, g1b, gs1b, _ = pt.debug_sample_lobes(m, s, si[r:r + 1], sf[r:r + 1], ss[r:r + 1])
            e1 = pt.debug_eval_bsdf(m, s, ei[r:r + 1])
            what = (name, mode, r)
            assert np.array_equal(g1.view(np.uint32), g[r:r + 1].view(np.uint32)) and gs1[0] == gs[r] and gs1b[0] == gs[r], what
            assert np.array_equal(g1b.view(np.uint32), g[r:r + 1].view(np.uint32)) and np.array_equal(l1.view(np.uint32), lobes[r:r + 1].view(np.uint32)), what
            assert np.array_equal(e1.view(np.uint32), e[r:r + 1].view(np.uint32)), what
