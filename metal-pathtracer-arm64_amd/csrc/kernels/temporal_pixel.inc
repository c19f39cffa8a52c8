// The body of k_temporal_accumulate (PTR_TEMPORAL_COV 0) and of k_temporal_accumulate_cov (PTR_TEMPORAL_COV 1): temporal.hip includes this
// file once inside each.  It is one text and not one inlined function because the plain kernel has to stay, instruction for instruction,
// the kernel it was before the covariance rule existed (profiles/temporal_cov_asm_diff.txt): with PTR_TEMPORAL_COV 0 the compiler sees
// the tokens it always saw, whereas the same body inlined from a function, or its predicates taken out into functions, already came out
// with other registers and operand orders.  Steps: include/ptr_temporal.h; under PTR_TEMPORAL_COV: include/ptr_temporal_cov.h.
// In scope: the kernel's parameters, and under PTR_TEMPORAL_COV `cv` (CovIo).
    const uint32_t i = blockIdx.x * kTemporalBlock + threadIdx.x;
    if (i >= width * height) return;
    const size_t at = static_cast<size_t>(i) * 3u;
    const f3 c = mk3(rgb[at], rgb[at + 1u], rgb[at + 2u]);   // (read before `out`, which may be the same buffer, is written)
#if PTR_TEMPORAL_COV
    float Cc[6], outCov[6];
    {
        const float2 c0 = cv.cov[at], c1 = cv.cov[at + 1u], c2 = cv.cov[at + 2u];   // (likewise read before outCov is written)
        const float raw[6] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y};
#pragma unroll
        for (int j = 0; j < 6; ++j) outCov[j] = Cc[j] = __builtin_isfinite(raw[j]) ? raw[j] : 0.0f;   // step 2 and every reset: out_cov = Cc
    }
#endif
    const float4 r0 = buf.r0[i], r2 = buf.r2[i];
    f3 result = c;
    float length = 1.0f;
    if (__float_as_uint(r2.w) == kMissWord || !finite3(c)) {
        length = 0.0f;   // step 1
#if PTR_TEMPORAL_COV
#pragma unroll
        for (int j = 0; j < 6; ++j) outCov[j] = 0.0f;
#endif
    } else if (hasHistory) {
        const float4 r1 = buf.r1[i];
        const f3 xPrev = mk3(r2), n = mk3(r1);
        const float w = static_cast<float>(width), h = static_cast<float>(height);
        float fcx, fcy, fpx, fpy;
        if (project(cur, mk3(r0), w, h, fcx, fcy) && project(prev, xPrev, w, h, fpx, fpy)) {
            const uint32_t px = i % width, py = i / width;
            const float sx = static_cast<float>(px) + (fpx - fcx), sy = static_cast<float>(py) + (fpy - fcy);
            if (__builtin_isfinite(sx) && __builtin_isfinite(sy)) {
                const float x0 = floorf(sx), y0 = floorf(sy);
                const float ax = sx - x0, ay = sy - y0;
                const float bx[2] = {1.0f - ax, ax}, by[2] = {1.0f - ay, ay};
                const f3 toCamera = xPrev - prev.o;
                const float bound = planeTolerance * sqrtf(dot(toCamera, toCamera));
                float B = 0.0f, Sn = 0.0f;
                f3 Sc = mk3(0.0f);
#if PTR_TEMPORAL_COV
                float Sv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#endif
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float b = bx[k & 1] * by[k >> 1];
                    const float tx = x0 + static_cast<float>(k & 1), ty = y0 + static_cast<float>(k >> 1);
                    if (!(b > 0.0f && tx >= 0.0f && tx < w && ty >= 0.0f && ty < h)) continue;
                    const uint32_t q = static_cast<uint32_t>(ty) * width + static_cast<uint32_t>(tx);
                    const float4 hq = buf.history[q], q0 = buf.prevR0[q], q1 = buf.prevR1[q];
#if PTR_TEMPORAL_COV
                    const float4 va = cv.historyA[q];   // (with the other three, before the predicate needs any of them)
                    const float2 vb = cv.historyB[q];
#endif
                    const f3 nq = mk3(q1);
                    const bool counts = hq.w >= 1.0f && finite3(mk3(hq)) && __float_as_uint(q0.w) == __float_as_uint(r0.w) &&
                                        dot(nq, n) >= normalCos && fabsf(dot(xPrev - mk3(q0), nq)) <= bound;
                    if (!counts) continue;
                    B = B + b;
                    Sc = Sc + b * mk3(hq);
                    Sn = Sn + b * hq.w;
#if PTR_TEMPORAL_COV
                    const float v[6] = {va.x, va.y, va.z, va.w, vb.x, vb.y};
#pragma unroll
                    for (int j = 0; j < 6; ++j) Sv[j] = Sv[j] + b * v[j];
#endif
                }
                if (B > 0.0f) {
                    const f3 hist = Sc / B;
                    const float N = Sn / B;
                    const float grown = N + 1.0f;
#if PTR_TEMPORAL_COV
                    float H[6];
#pragma unroll
                    for (int j = 0; j < 6; ++j) H[j] = Sv[j] / B;
                    const float d = lum(c) - lum(hist);
                    const float V = lumvar(Cc) + lumvar(H);
                    if (!(cv.rejectSigma > 0.0f && d * d > (cv.rejectSigma * cv.rejectSigma) * V)) {   // else the consistency test resets
#endif
                    length = grown < maxHistory ? grown : maxHistory;
                    const float a = 1.0f / length;
                    result = hist + (c - hist) * a;
#if PTR_TEMPORAL_COV
                    const float k1 = 1.0f - a;
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        const float blended = (k1 * k1) * H[j] + (a * a) * Cc[j];
                        outCov[j] = __builtin_isfinite(blended) ? blended : Cc[j];
                    }
                    }
#endif
                }
            }
        }
    }
    buf.historyOut[i] = mk4(result, length);
    out[at] = result.x;
    out[at + 1u] = result.y;
    out[at + 2u] = result.z;
    if (outLength) outLength[i] = length;
#if PTR_TEMPORAL_COV
    cv.historyAOut[i] = make_float4(outCov[0], outCov[1], outCov[2], outCov[3]);   // step 7
    cv.historyBOut[i] = make_float2(outCov[4], outCov[5]);
    cv.outCov[at] = make_float2(outCov[0], outCov[1]);
    cv.outCov[at + 1u] = make_float2(outCov[2], outCov[3]);
    cv.outCov[at + 2u] = make_float2(outCov[4], outCov[5]);
#endif
