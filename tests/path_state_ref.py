"""A float64 statement of what carries a path from one vertex to the next: the bookkeeping between the traversal, the light samples and the
BSDF sample, which csrc/kernels/wavefront.hip (shadeSlot) and oracle/oracle_integrator.cpp (render) each state in float32.  Written from
the reference's render loops (shaders/pathtrace.metal:5768-5773 the medium stack, 5869-5876 Beer-Lambert over the segment inside the
innermost medium, 6694-6709 push / overwrite-when-full / pop / pop-at-zero; src/headless/EmbreeHeadlessRenderer.mm:2599-2601 the initial
state, 2660-2706 the emitter hit and its MIS weight, the escaped ray before it, 3098-3120 throughput, clamp, the two termination tests,
lastBsdfPdf, roulette).  Bookkeeping only: a vertex's facts (hit or miss, t, material, front face, geometric normal) and its BSDF sample
are inputs.  Vectorised over paths; every float is float64.

The wavefront keeps the same state packed: the flags word (csrc/kernels/device_types.h kFlag*), eight 16-bit material ids in one uint4,
and radiance that reaches `accum` one visit after it was queued (accum_schedule)."""
import numpy as np

import light_ref as lr

MAX_STACK = 8
REC_SLOTS = 5
MIS_MIN, MIS_MAX = 1.0e-4, 0.9999
ROULETTE_FROM = 5           # no draw before this depth
ROULETTE_LO, ROULETTE_HI = 0.05, 0.95
DEPTH_MASK = 0x1FF          # two 9-bit counters: the device clamps maxDepth to 511
LUMA = np.array([0.2126, 0.7152, 0.0722])


# ---------------------------------------------------------------- the flags word
_FIELDS = (("alive", 0, 1), ("last_delta", 1, 1), ("flush", 2, 1), ("walk", 3, 1), ("medium_depth", 4, 4), ("depth", 8, 9), ("spec_depth", 17, 9),
           ("pending", 26, 5), ("spare", 31, 1))


def decode_flags(word):
    """field -> value of the flags word(s) (ray1.w): alive, last_delta, flush, walk (1 bit each), medium_depth (4 bits), depth and
    spec_depth (9 bits each), pending (5 bits, bit k: record slot k), spare (bit 31, never set)."""
    w = np.asarray(word, np.uint64)
    return {name: ((w >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.uint32) for name, shift, bits in _FIELDS}


def encode_flags(**fields):
    """the inverse of decode_flags; a value that does not fit its field is an error, not a carry into the next one"""
    word = np.zeros(np.broadcast(*[np.asarray(v) for v in fields.values()]).shape, np.uint64)
    for name, shift, bits in _FIELDS:
        v = np.asarray(fields.get(name, 0), np.uint64)
        assert np.all(v < (1 << bits)), name
        word |= v << np.uint64(shift)
    return word.astype(np.uint32)


# ---------------------------------------------------------------- the medium stack, packed
def pack_stack(ids):
    """[..., 8] material ids (each < 2^16) -> [..., 4] uint32: entry i in word i // 2, bits 16 (i % 2) .. 16 (i % 2) + 15"""
    ids = np.asarray(ids, np.uint64)
    assert ids.shape[-1] == MAX_STACK and np.all(ids < 65536)
    return (ids[..., 0::2] | (ids[..., 1::2] << np.uint64(16))).astype(np.uint32)


def unpack_stack(words):
    """[..., 4] uint32 -> [..., 8] ids"""
    w = np.asarray(words, np.uint32)
    out = np.zeros(w.shape[:-1] + (MAX_STACK,), np.uint32)
    out[..., 0::2] = w & 0xFFFF
    out[..., 1::2] = w >> 16
    return out


def stack_event(stack, depth, event, material):
    """(stack [n, 8], depth [n]) after a medium event [n] (+1 push `material`, -1 pop, 0 none): a push onto a full stack overwrites its
    top and leaves the depth, a pop of an empty one does nothing."""
    stack, depth = np.array(stack, np.int64), np.array(depth, np.int64)
    push, pop = event > 0, event < 0
    at = np.minimum(depth, MAX_STACK - 1)
    rows = np.flatnonzero(push)
    stack[rows, at[rows]] = np.asarray(material, np.int64)[rows]
    depth = np.where(push, np.minimum(depth + 1, MAX_STACK), np.where(pop & (depth > 0), depth - 1, depth))
    return stack, depth


def medium_event(non_thin_dielectric, direction, stored_normal, front):
    """What the samplers report beside a dielectric sample (pathtrace.metal:5683): a direction that crosses the geometric surface of a
    dielectric that is not thin-walled is +1 from the front and -1 from the back.  stored_normal: the outward geometric normal."""
    facing = np.where(np.asarray(front, bool)[:, None], stored_normal, -np.asarray(stored_normal, np.float64))
    crosses = np.einsum("ij,ij->i", np.asarray(direction, np.float64), facing) < 0.0
    return np.where(np.asarray(non_thin_dielectric, bool) & crosses, np.where(front, 1, -1), 0)


# ---------------------------------------------------------------- clamps and weights
class Clamps:
    """MakeFireflyParams (EmbreeHeadlessRenderer.mm:381-391) of the settings"""

    def __init__(self, s):
        self.enabled = bool(s.fireflyClampEnabled)
        self.factor, self.floor = max(float(s.fireflyClampFactor), 0.0), max(float(s.fireflyClampFloor), 0.0)
        self.throughput = max(float(s.throughputClamp), 0.0)
        self.metal = bool(s.metalSemantics & 64)
        self.max_contribution = max(float(s.fireflyClampMaxContribution), 0.0)


def clamp_throughput(thr, c):
    """ClampPathThroughput: not finite -> 0; with the clamp on and a positive limit, a luminance above it is scaled down to it"""
    thr = np.array(thr, np.float64)
    bad = ~np.isfinite(thr).all(axis=1)
    thr[bad] = 0.0
    if not c.enabled or c.throughput <= 0.0:
        return thr, np.zeros(len(thr), bool)
    lum = np.maximum(thr, 0.0) @ LUMA
    over = (lum > c.throughput) & (lum > 0.0)
    return np.where(over[:, None], thr * (c.throughput / np.maximum(lum, 1e-6))[:, None], thr), over


def clamp_firefly(thr, contribution, c):
    """ClampFireflyContribution: throughput x contribution, negatives to 0, its luminance held to max(luminance(throughput) factor, floor)"""
    combined = np.asarray(thr, np.float64) * np.asarray(contribution, np.float64)
    bad = ~np.isfinite(combined).all(axis=1)
    positive = np.maximum(combined, 0.0)
    if c.enabled:
        lum = positive @ LUMA
        limit = np.maximum((np.maximum(thr, 0.0) @ LUMA) * c.factor, c.floor)
        if c.metal and c.max_contribution > 0.0:
            limit = np.maximum(limit, c.max_contribution)
        over = (lum > limit) & (lum > 0.0)
        positive = np.where(over[:, None], np.maximum(combined * (limit / np.maximum(lum, 1e-6))[:, None], 0.0), positive)
    return np.where(bad[:, None], 0.0, positive)


def bsdf_side_mis(settings, last_delta, last_pdf, light_pdf, lights_sampled):
    """The weight of radiance a BSDF-sampled ray runs into (an escaped ray under a sampled environment, an emitter among rectangle
    lights): 1.0 unless the last bounce was not a delta one, or specular NEE or MNEE is on - and then lastPdf / (lastPdf + lightPdf),
    1.0 when that sum is not positive, clamped to [1e-4, 0.9999]."""
    last_pdf, light_pdf = np.asarray(last_pdf, np.float64), np.asarray(light_pdf, np.float64)
    use = (~np.asarray(last_delta, bool)) | bool(settings.enableSpecularNee) | bool(settings.enableMnee)
    denom = last_pdf + light_pdf
    with np.errstate(invalid="ignore", divide="ignore"):
        mis = np.clip(np.where(denom > 0.0, last_pdf / np.where(denom > 0.0, denom, 1.0), 1.0), MIS_MIN, MIS_MAX)
    return np.where(use & bool(lights_sampled), mis, 1.0)


# ---------------------------------------------------------------- one vertex
def initial_state(n, rng):
    return dict(throughput=np.ones((n, 3)), last_pdf=np.ones(n), last_delta=np.ones(n, bool), spec_depth=np.zeros(n, np.int64),
                depth=np.zeros(n, np.int64), medium_depth=np.zeros(n, np.int64), stack=np.zeros((n, MAX_STACK), np.int64),
                rng=np.asarray(rng, np.uint32).copy())


def attenuation(state, t, sigma_of_material, media):
    """Beer-Lambert over the segment just travelled, by the absorption of the innermost medium (the stack's top entry)"""
    n = len(t)
    inside = np.where(state["medium_depth"] > 0, state["stack"][np.arange(n), np.maximum(state["medium_depth"] - 1, 0)], 0)   # (an empty stack is not read)
    sigma = np.maximum(np.asarray(sigma_of_material, np.float64)[inside], 0.0)
    on = media & (state["medium_depth"] > 0) & (sigma > 0.0).any(axis=1)
    return np.where(on[:, None], np.exp(-sigma * np.maximum(np.asarray(t, np.float64), 0.0)[:, None]), 1.0), sigma, on


def step(settings, state, vertex, sample, sigma_of_material):
    """The state after a surface vertex that takes a BSDF sample (no emitter, no miss), and how the path fares there.
    state: initial_state's fields before the vertex (rng: after the vertex's light samples and its BSDF sample).
    vertex: t [n], material [n] (clamped index), and what the vertex itself adds to the sample's weight: nothing.
    sample: weight [n, 3], pdf [n], is_delta [n], medium_event [n], valid [n] (pdf > 0, a direction, a finite weight).
    Returns (state after, info): info has ended [n] with its reason - 'invalid', 'throughput' (not finite, or no positive component),
    'roulette', 'depth' -, attenuation [n, 3], clamped [n], roulette_taken / roulette_draw / roulette_threshold [n]."""
    n = len(vertex["t"])
    media = bool(settings.metalSemantics & 1)
    c = Clamps(settings)
    att, _, _ = attenuation(state, vertex["t"], sigma_of_material, media)
    thr = state["throughput"] * att
    valid = np.asarray(sample["valid"], bool)
    event = np.where(valid & media, sample["medium_event"], 0)
    stack, medium_depth = stack_event(state["stack"], state["medium_depth"], event, vertex["material"])
    spec_depth = np.where(valid, np.where(sample["is_delta"], state["spec_depth"] + 1, 0), state["spec_depth"])
    thr = np.where(valid[:, None], thr * np.asarray(sample["weight"], np.float64), thr)
    thr, clamped = clamp_throughput(thr, c)
    max_comp = thr.max(axis=1)
    dead = valid & (~np.isfinite(thr).all(axis=1) | ~(max_comp > 0.0))
    goes = valid & ~dead
    last_pdf = np.where(goes & (np.asarray(sample["pdf"]) > 0.0), sample["pdf"], state["last_pdf"])
    last_delta = np.where(goes, np.asarray(sample["is_delta"], bool), state["last_delta"])
    # roulette: from depth 5 on, one draw against clamp(maxComp, 0.05, 0.95); survival divides by it
    taken = goes & bool(settings.enableRussianRoulette) & (state["depth"] >= ROULETTE_FROM)
    draws, after = lr.rng_draw(state["rng"], 1)
    threshold = np.clip(max_comp, ROULETTE_LO, ROULETTE_HI)
    killed = taken & (draws[:, 0] > threshold)
    thr = np.where((taken & ~killed)[:, None], thr / threshold[:, None], thr)
    rng = np.where(taken, after, state["rng"]).astype(np.uint32)
    depth = state["depth"] + 1
    max_depth = min(int(settings.maxDepth), DEPTH_MASK)
    out_of_depth = depth >= max_depth
    ended = ~valid | dead | killed | out_of_depth
    reason = np.where(~valid, "invalid", np.where(dead, "throughput", np.where(killed, "roulette", np.where(out_of_depth, "depth", ""))))
    new = dict(throughput=thr, last_pdf=last_pdf, last_delta=last_delta, spec_depth=spec_depth, depth=depth, medium_depth=medium_depth,
               stack=stack, rng=rng)
    info = dict(ended=ended, reason=reason, attenuation=att, clamped=clamped & valid, roulette_taken=taken, roulette_draw=draws[:, 0],
                roulette_threshold=threshold, roulette_killed=killed, medium_event=event)
    return new, info


def escaped(settings, state, background, env_pdf=0.0, env_sampled=False):
    """radiance of a ray that leaves the scene: the background, weighted against environment sampling, through the firefly clamp"""
    mis = bsdf_side_mis(settings, state["last_delta"], state["last_pdf"], env_pdf, env_sampled)
    return clamp_firefly(state["throughput"], np.asarray(background, np.float64) * np.asarray(mis)[:, None], Clamps(settings))


def emitter(settings, state, emission, light_pdf=0.0, lights_sampled=False):
    """radiance of an emitter a BSDF-sampled ray hits, weighted against rectangle-light sampling"""
    mis = bsdf_side_mis(settings, state["last_delta"], state["last_pdf"], light_pdf, lights_sampled)
    return clamp_firefly(state["throughput"], np.asarray(emission, np.float64) * np.asarray(mis)[:, None], Clamps(settings))


# ---------------------------------------------------------------- when radiance arrives
def accum_schedule(immediate, queued, ends_at):
    """The wavefront's `accum` of one path after every iteration.  immediate, queued [v, 3]: what vertex k adds at once (emission,
    background) and what it queues as light connections (they land at the slot's next visit); ends_at: the vertex the path ends at.
    Returns (accum [ends_at + 2, 3] after iterations 0 .. ends_at + 1, the iteration the item is published at, flushed): after iteration
    k < ends_at accum holds the immediate terms of vertices 0..k and the queued terms of 0..k-1.  A path that ends with connections
    outstanding is flagged and published one visit later (accum then reads 0: it was handed on); otherwise it is published at once."""
    immediate, queued = np.asarray(immediate, np.float64), np.asarray(queued, np.float64)
    rows = []
    for k in range(ends_at + 1):
        rows.append(immediate[: k + 1].sum(axis=0) + queued[:k].sum(axis=0))
    flushed = bool((queued[ends_at] != 0.0).any())
    total = immediate[: ends_at + 1].sum(axis=0) + queued[: ends_at + 1].sum(axis=0)
    if not flushed:
        rows[ends_at] = np.zeros(3)
    rows.append(np.zeros(3))
    return np.array(rows), ends_at + (1 if flushed else 0), flushed, total
