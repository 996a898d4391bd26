// Resampling of a learned position table, fp32 [prefix + Hs*Ws, C] -> [prefix + Ho*Wo, C], channels last as the parameter is stored, and the transposed
// map for its gradient.  ocn_pos_resample_fwd is F.interpolate(grid, size=(Ho, Wo), mode, antialias, align_corners=False) per channel (what the
// reference's resize_pos_embed / resize_text_pos_embed call, model.py:790-854); ocn_pos_resample_bwd is dsrc = W^T ddst.  The prefix rows (class token)
// are copied by both.
//
// Per axis, length n -> R, every output index r owns a list of taps (source index, weight), built from integers -- with c2 = n (2r + 1):
//   antialiased    M = max(n, R), K = 2 (cubic) or 1 (linear): taps k in [max(0, (c2 - 2KM + R) / 2R), min(n, (c2 + 2KM + R) / 2R)) (C division), raw weight
//                  f(((2k + 1) R - c2) / 2M), f = Keys' cubic with a = -0.5 or the triangle; the weight is raw / S, S = the raw weights added in tap order
//   cubic          num = c2 - R, f0 = floor(num / 2R), tn = num - 2R f0: four taps clamp(f0 - 1 + j, 0, n - 1), j = 0..3, weight cubic(((j - 1) 2R - tn) / 2R)
//                  with a = -0.75, not renormalised; taps clamped onto one border element stay separate terms of the sum
//   linear         num = max(c2 - R, 0), f0 = min(num / 2R, n - 1), tn = num - 2R f0: taps f0 with (2R - tn) / 2R and min(f0 + 1, n - 1) with tn / 2R
// Every numerator is an exact integer below 2^24; the one fp32 division per weight argument is the only rounding in a tap position.  A tap whose weight
// is exactly 0 is dropped from the list: an axis with n == R is the list {(r, 1.0f)} under all three rules, and the result is the source's bits.
//
// One workgroup per row of the result, lanes along C (float4 where C % 4 == 0 and both tables are 16-byte aligned, else scalar):
//   fwd   result row (oy, ox):  dst = sum_a wy[a] * (sum_b wx[b] * src[iy[a], ix[b]])
//   bwd   result row (sy, sx):  the lists are the OUTPUTS whose taps hold the row / the column, in increasing output index, each with the weight the
//         forward gives that source element (several clamped taps of one output added in tap order): dsrc = sum_a cy[a] * (sum_b cx[b] * ddst[oy[a], ox[b]])
// both sums in list order, the inner one first, each started with its first product (no zero is added), in fp32 (fused multiply-adds): the same additions
// in the same order in every run -- gather form, no atomic anywhere, the same bits every time.  An empty list (a source element no output reads) gives 0.
#include "ocn_common.h"

namespace {

constexpr int PR_TAPS = 64;                         // entries of a list: taps of an output (<= n <= 64 antialiased), outputs that read a source element
constexpr int PR_MAX_SIDE = 64, PR_MAX_LEN = 4096;  // a grid side; the length of a 1-D linear call (two taps whatever the length)

struct PrAxis {
    int n, R, cubic, aa;
};
// the taps of one output index: `cnt` of them; tap j has source index lo + j (antialiased) or the clamped index of its rule, and the argument
// (num0 + j * step) / den of its weight function
struct PrWin {
    int lo, cnt, num0, step, den;
};

// Keys' cubic convolution kernel with parameter a (torch's two pieces: a = -0.5 antialiased, -0.75 otherwise)
OCN_DEV float pr_cubic(float x, float a) {
    x = fabsf(x);
    if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return ((a * x - 5.0f * a) * x + 8.0f * a) * x - 4.0f * a;
    return 0.0f;
}

OCN_DEV PrWin pr_window(const PrAxis ax, int r) {
    const int n = ax.n, R = ax.R, c2 = n * (2 * r + 1);  // below 2^26
    PrWin w;
    if (ax.aa) {
        const int M = max(n, R), K = ax.cubic ? 2 : 1;
        w.lo = max(0, (c2 - 2 * K * M + R) / (2 * R));  // a negative numerator truncates towards 0: at most 0 either way
        w.cnt = min(min(n, (c2 + 2 * K * M + R) / (2 * R)) - w.lo, PR_TAPS);
        w.num0 = (2 * w.lo + 1) * R - c2;
        w.step = 2 * R;
        w.den = 2 * M;
    } else {
        const int den = 2 * R, num = ax.cubic ? c2 - R : max(c2 - R, 0);
        const int f0 = num >= 0 ? min(num / den, n - 1) : -((-num + den - 1) / den);  // floor
        w.lo = f0;
        w.cnt = ax.cubic ? 4 : 2;
        w.num0 = num - f0 * den;  // tn, in [0, 2R)
        w.step = 0;
        w.den = den;
    }
    return w;
}

// tap j of a window: its raw weight and, in `idx`, its source index
OCN_DEV float pr_tap(const PrAxis ax, const PrWin w, int j, int& idx) {
    const float den = (float)w.den;
    if (ax.aa) {
        idx = w.lo + j;
        const float x = (float)(w.num0 + j * w.step) / den;
        return ax.cubic ? pr_cubic(x, -0.5f) : fmaxf(0.0f, 1.0f - fabsf(x));
    }
    if (ax.cubic) {
        idx = ocn_clamp_index(w.lo - 1 + j, ax.n);
        return pr_cubic((float)((j - 1) * w.den - w.num0) / den, -0.75f);
    }
    idx = min(w.lo + j, ax.n - 1);
    return (float)(j == 0 ? w.den - w.num0 : w.num0) / den;
}

// the weight output r gives source element s: its taps on s, each divided by the window's sum where the rule normalises, added in tap order
OCN_DEV float pr_coef(const PrAxis ax, int r, int s) {
    const PrWin w = pr_window(ax, r);
    float S = 1.0f, c = 0.0f;
    int idx;
    if (ax.aa) {
        S = 0.0f;
        for (int j = 0; j < w.cnt; ++j) S += pr_tap(ax, w, j, idx);
    }
    for (int j = 0; j < w.cnt; ++j) {
        const float raw = pr_tap(ax, w, j, idx);
        if (idx == s) c += ax.aa ? raw / S : raw;
    }
    return c;
}

// BWD = false: `out` is dst, one row per (oy, ox) of the Ro x Co = Ho x Wo grid, read from `in` = src with the Ri x Ci = Hs x Ws grid.
// BWD = true:  `out` is dsrc, one row per (sy, sx) of the Ro x Co = Hs x Ws grid, read from `in` = ddst with the Ri x Ci = Ho x Wo grid.
// ay / ax: the forward's axes (n = source length, R = output length) either way.
template <bool BWD>
__global__ __launch_bounds__(256) void pos_resample_kernel(const float* __restrict__ in, float* __restrict__ out, int prefix, int Ro, int Co, int Ci,
                                                           PrAxis ay, PrAxis ax, int C, int vec) {
    __shared__ float raw[2][PR_TAPS], lw[2][PR_TAPS];
    __shared__ int ridx[2][PR_TAPS], li[2][PR_TAPS], cnt[2];
    const int tid = threadIdx.x, row = blockIdx.x;
    if (row < prefix) {  // the class-token rows: copied
        for (int c = tid; c < C; c += 256) out[(size_t)row * C + c] = in[(size_t)row * C + c];
        return;
    }
    const int oy = (row - prefix) / Co, ox = (row - prefix) - oy * Co;
    (void)Ro;

    // ---- the two lists: candidates by threads 0..63 (rows) and 64..127 (columns), then one thread per axis normalises and drops the zeros ----
    if (tid < 2 * PR_TAPS) {
        const int a = tid >> 6, j = tid & 63;
        const PrAxis axis = a == 0 ? ay : ax;
        const int o = a == 0 ? oy : ox;
        float v = 0.0f;
        int idx = 0;
        if (BWD) {  // candidate j = output index j
            if (j < axis.R) v = pr_coef(axis, j, o);
            idx = j;
        } else {    // candidate j = tap j of this output
            const PrWin w = pr_window(axis, o);
            if (j < w.cnt) v = pr_tap(axis, w, j, idx);
        }
        raw[a][j] = v;
        ridx[a][j] = idx;
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {
        const int a = tid >> 6;
        const PrAxis axis = a == 0 ? ay : ax;
        const int m = BWD ? min(axis.R, PR_TAPS) : pr_window(axis, a == 0 ? oy : ox).cnt;
        const bool normalise = !BWD && axis.aa;  // (pr_coef has divided already, by the same weights added in the same order)
        float S = 0.0f;
        for (int j = 0; normalise && j < m; ++j) S += raw[a][j];  // tap order
        int k = 0;
        for (int j = 0; j < m; ++j) {
            const float w = normalise ? raw[a][j] / S : raw[a][j];
            if (w != 0.0f) {
                lw[a][k] = w;
                li[a][k] = ridx[a][j];
                ++k;
            }
        }
        cnt[a] = k;
    }
    __syncthreads();

    const int na = cnt[0], nb = cnt[1];
    float* __restrict__ o = out + (size_t)row * C;
    const float* __restrict__ grid = in + (size_t)prefix * C;
    const int C4 = vec ? C >> 2 : 0;
    for (int c4 = tid; c4 < C4; c4 += 256) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (nb > 0) {
            for (int a = 0; a < na; ++a) {
                const float* __restrict__ p = grid + (size_t)li[0][a] * Ci * C + 4 * c4;
                f32x4 rs = lw[1][0] * *(const f32x4*)(p + (size_t)li[1][0] * C);
                for (int b = 1; b < nb; ++b) rs += lw[1][b] * *(const f32x4*)(p + (size_t)li[1][b] * C);
                acc = a == 0 ? lw[0][0] * rs : acc + lw[0][a] * rs;
            }
        }
        *(f32x4*)(o + 4 * c4) = acc;
    }
    for (int c = 4 * C4 + tid; c < C; c += 256) {
        float acc = 0.f;
        if (nb > 0) {
            for (int a = 0; a < na; ++a) {
                const float* __restrict__ p = grid + (size_t)li[0][a] * Ci * C + c;
                float rs = lw[1][0] * p[(size_t)li[1][0] * C];
                for (int b = 1; b < nb; ++b) rs += lw[1][b] * p[(size_t)li[1][b] * C];
                acc = a == 0 ? lw[0][0] * rs : acc + lw[0][a] * rs;
            }
        }
        o[c] = acc;
    }
}

int pos_resample(const char* name, bool bwd, const float* in, float* out, int prefix, int Hs, int Ws, int Ho, int Wo, int C, int mode, int antialias,
                 ocn_stream_t stream) {
    OCN_CHECK_ARG(in && out, "%s: null operand", name);
    OCN_CHECK_ARG((((uintptr_t)in | (uintptr_t)out) & 3) == 0, "%s: the tables must be 4-byte aligned", name);
    OCN_CHECK_ARG(mode == 0 || mode == 1, "%s: mode=%d must be 0 (linear) or 1 (cubic)", name, mode);
    OCN_CHECK_ARG(antialias == 0 || antialias == 1, "%s: antialias=%d must be 0 or 1", name, antialias);
    OCN_CHECK_ARG(prefix >= 0 && prefix <= PR_MAX_SIDE, "%s: prefix=%d must lie in [0, %d]", name, prefix, PR_MAX_SIDE);
    OCN_CHECK_ARG(C >= 1 && C <= (1 << 20), "%s: C=%d must lie in [1, 2^20]", name, C);
    const bool oned = Hs == 1 && Ho == 1;  // the text table: a row of positions
    OCN_CHECK_ARG(!(oned && mode == 0 && antialias), "%s: antialias=1 is not defined for a 1-D linear call (Hs = Ho = 1)", name);
    if (oned && mode == 0 && !bwd) {
        OCN_CHECK_ARG(Ws >= 1 && Ws <= PR_MAX_LEN && Wo >= 1 && Wo <= PR_MAX_LEN, "%s: 1-D lengths Ws=%d Wo=%d must lie in [1, %d]", name, Ws, Wo,
                      PR_MAX_LEN);
    } else {
        OCN_CHECK_ARG(Hs >= 1 && Hs <= PR_MAX_SIDE && Ws >= 1 && Ws <= PR_MAX_SIDE, "%s: source grid Hs=%d Ws=%d: sides must lie in [1, %d]", name, Hs, Ws,
                      PR_MAX_SIDE);
        OCN_CHECK_ARG(Ho >= 1 && Ho <= PR_MAX_SIDE && Wo >= 1 && Wo <= PR_MAX_SIDE, "%s: output grid Ho=%d Wo=%d: sides must lie in [1, %d]", name, Ho, Wo,
                      PR_MAX_SIDE);
    }
    const PrAxis ay = {Hs, Ho, mode, antialias}, ax = {Ws, Wo, mode, antialias};
    const int vec = (C & 3) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    if (bwd) {
        hipLaunchKernelGGL(pos_resample_kernel<true>, dim3((unsigned)(prefix + Hs * Ws)), dim3(256), 0, (hipStream_t)stream, in, out, prefix, Hs, Ws, Wo, ay,
                           ax, C, vec);
    } else {
        hipLaunchKernelGGL(pos_resample_kernel<false>, dim3((unsigned)(prefix + Ho * Wo)), dim3(256), 0, (hipStream_t)stream, in, out, prefix, Ho, Wo, Ws,
                           ay, ax, C, vec);
    }
    OCN_CHECK_LAUNCH(name);
    return OCN_OK;
}

}  // namespace

extern "C" int ocn_pos_resample_fwd(const float* src, float* dst, int prefix, int Hs, int Ws, int Ho, int Wo, int C, int mode, int antialias,
                                    ocn_stream_t stream) {
    return pos_resample("ocn_pos_resample_fwd", false, src, dst, prefix, Hs, Ws, Ho, Wo, C, mode, antialias, stream);
}

extern "C" int ocn_pos_resample_bwd(const float* ddst, float* dsrc, int prefix, int Hs, int Ws, int Ho, int Wo, int C, int mode, int antialias,
                                    ocn_stream_t stream) {
    return pos_resample("ocn_pos_resample_bwd", true, ddst, dsrc, prefix, Hs, Ws, Ho, Wo, C, mode, antialias, stream);
}
