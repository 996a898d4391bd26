// Colour jitter and grayscale on the device (reference transform.py:335-364 and :442-450: color_jitter(*aug_cfg.color_jitter, p) and
// gray_scale(p) of the train transform, between RandomResizedCrop and ToTensor).  The parameters are drawn on the host
// (input_pipeline.color_jitter_plan) and travel with the batch; nothing is read back.  The arithmetic is defined in include/openclip_hip.h.
//
// Two launches:
//   mean   one workgroup per image whose plan holds a contrast step (every other workgroup leaves on a uniform branch): the steps in front of the
//          contrast step per pixel on the fly, gray quantised to 2^-24 and summed in INTEGERS -- the sum does not depend on the order of its terms,
//          so neither the launch nor the alignment of the image can change mean_ws[b];
//   apply  the whole chain per pixel.  A workgroup belongs to ONE image (its parameters are wave-uniform: the step loop branches on scalars, only
//          the hue sector select is per lane) and covers CJ_WG_ITEMS items of it.
// Items of an image (cj_split): `head` single pixels until the byte address is a multiple of 4, then groups of 4 pixels = 12 bytes = three aligned
// dwords, then up to 3 single pixels.  A single pixel goes by byte accesses, a group by dword accesses where the pointer is aligned like the one the
// split was made for, by bytes elsewhere; both forms fill the same three registers and run the same arithmetic.
// No address depends on factors or plan: whatever they hold, the kernels read and write exactly B * H * W * 3 bytes.
#include "ocn_common.h"

namespace {

constexpr int CJ_THREADS = 256;
constexpr int CJ_ITEMS = 4;                          // items per thread of the apply pass: their loads are in flight together
constexpr int CJ_WG_ITEMS = CJ_THREADS * CJ_ITEMS;   // 1024 items: 4096 pixels of an aligned image
constexpr int CJ_MAX_SIDE = 8192;
constexpr float CJ_MEAN_ONE = 16777216.0f;           // 2^24: the quantum of the contrast mean's terms is 2^-24

struct CjSplit {
    int head, ngroups, nitems;
};
OCN_DEV CjSplit cj_split(uintptr_t base, int npix) {
    CjSplit s;
    s.head = min((int)(base & 3), npix);  // pixel k starts at base + 3k: base + 3 head = base + 4 head - head is a multiple of 4
    const int rem = npix - s.head;
    s.ngroups = rem >> 2;
    s.nitems = s.ngroups + s.head + (rem & 3);
    return s;
}

// item t of an image at p into three registers: a group's 12 bytes, or one pixel in the low 24 bits of w[0]
OCN_DEV void cj_load_item(const uint8_t* p, const CjSplit& s, int t, bool dword, uint32_t w[3]) {
    if (t < s.ngroups) {
        const uint8_t* q = p + 3 * s.head + 12 * t;
        if (dword) {
#pragma unroll
            for (int i = 0; i < 3; ++i) w[i] = ((const uint32_t*)q)[i];
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                w[i] = (uint32_t)q[4 * i] | ((uint32_t)q[4 * i + 1] << 8) | ((uint32_t)q[4 * i + 2] << 16) | ((uint32_t)q[4 * i + 3] << 24);
        }
    } else {
        const int k = t - s.ngroups;  // the head's pixels first, then the tail's
        const uint8_t* q = p + 3 * (k < s.head ? k : 4 * s.ngroups + k);
        w[0] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
        w[1] = w[2] = 0u;
    }
}

OCN_DEV void cj_store_item(uint8_t* p, const CjSplit& s, int t, const uint32_t w[3]) {
    if (t < s.ngroups) {  // the split was made for this pointer: every group is dword-aligned
        uint32_t* q = (uint32_t*)(p + 3 * s.head + 12 * t);
#pragma unroll
        for (int i = 0; i < 3; ++i) q[i] = w[i];
    } else {
        const int k = t - s.ngroups;
        uint8_t* q = p + 3 * (k < s.head ? k : 4 * s.ngroups + k);
        q[0] = (uint8_t)w[0];
        q[1] = (uint8_t)(w[0] >> 8);
        q[2] = (uint8_t)(w[0] >> 16);
    }
}

// 12 bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 -> x = u8 / 255 per channel of 4 pixels
OCN_DEV void cj_unpack(const uint32_t w[3], float r[4], float g[4], float b[4]) {
    float v[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = (float)((w[i >> 2] >> (8 * (i & 3))) & 255u) * (1.0f / 255.0f);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = v[3 * i], g[i] = v[3 * i + 1], b[i] = v[3 * i + 2];
}

// out = round-half-even(255 x), the one rounding
OCN_DEV void cj_pack(const float r[4], const float g[4], const float b[4], uint32_t w[3]) {
    uint32_t q[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        q[3 * i] = (uint32_t)__builtin_rintf(__builtin_amdgcn_fmed3f(255.0f * r[i], 0.f, 255.f));
        q[3 * i + 1] = (uint32_t)__builtin_rintf(__builtin_amdgcn_fmed3f(255.0f * g[i], 0.f, 255.f));
        q[3 * i + 2] = (uint32_t)__builtin_rintf(__builtin_amdgcn_fmed3f(255.0f * b[i], 0.f, 255.f));
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (q[4 * i] & 255u) | ((q[4 * i + 1] & 255u) << 8) | ((q[4 * i + 2] & 255u) << 16) | (q[4 * i + 3] << 24);
}

OCN_DEV float cj_clamp(float v) { return __builtin_amdgcn_fmed3f(v, 0.f, 1.f); }
OCN_DEV float cj_gray(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// rgb -> hsv, hh <- (hh + h) mod 1, hsv -> rgb; r, g, b in [0, 1] on entry and on exit
OCN_DEV void cj_hue(float& r, float& g, float& b, float h) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const float cr = maxc - minc;
    const bool eq = maxc == minc;
    const float s = cr * __builtin_amdgcn_rcpf(eq ? 1.0f : maxc);
    const float icr = __builtin_amdgcn_rcpf(eq ? 1.0f : cr);
    const float rc = (maxc - r) * icr, gc = (maxc - g) * icr, bc = (maxc - b) * icr;
    float hh = maxc == r ? bc - gc : (maxc == g ? 2.0f + rc - bc : 4.0f + gc - rc);
    hh = __builtin_amdgcn_fractf(hh * (1.0f / 6.0f) + 1.0f);
    hh = __builtin_amdgcn_fractf(hh + h);  // in [0, 1)
    const float h6 = 6.0f * hh, fi = __builtin_floorf(h6), f = h6 - fi;
    int i = (int)fi;
    i = i >= 6 ? i - 6 : i;
    const float v = maxc;
    const float p = cj_clamp(v * (1.0f - s)), q = cj_clamp(v * (1.0f - s * f)), t = cj_clamp(v * (1.0f - s * (1.0f - f)));
    r = (i == 0 || i == 5) ? v : (i == 1 ? q : (i == 4 ? t : p));
    g = (i == 1 || i == 2) ? v : (i == 0 ? t : (i == 3 ? q : p));
    b = (i == 3 || i == 4) ? v : (i == 2 ? t : (i == 5 ? q : p));
}

// steps [k0, k1) of a plan on 4 pixels; plan, fac and m are wave-uniform, so every branch but the selects inside cj_hue is a scalar one
OCN_DEV void cj_steps(float r[4], float g[4], float b[4], int plan, const float fac[4], float m, int k0, int k1) {
    for (int k = k0; k < k1; ++k) {
        const int code = (plan >> (3 * k)) & 7;
        if (code == 1) {
            const float f = fac[0];
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = cj_clamp(f * r[i]), g[i] = cj_clamp(f * g[i]), b[i] = cj_clamp(f * b[i]);
        } else if (code == 2) {
            const float f = fac[1], c = (1.0f - f) * m;
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = cj_clamp(f * r[i] + c), g[i] = cj_clamp(f * g[i] + c), b[i] = cj_clamp(f * b[i] + c);
        } else if (code == 3) {
            const float f = fac[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float c = (1.0f - f) * cj_gray(r[i], g[i], b[i]);
                r[i] = cj_clamp(f * r[i] + c), g[i] = cj_clamp(f * g[i] + c), b[i] = cj_clamp(f * b[i] + c);
            }
        } else if (code == 4) {
            const float h = fac[3];
#pragma unroll
            for (int i = 0; i < 4; ++i) cj_hue(r[i], g[i], b[i], h);
        }  // 0 and 5..7: nothing
    }
}

// index of the first contrast step of a plan, 4 when it has none
OCN_DEV int cj_first_contrast(int plan) {
    int kc = 4;
#pragma unroll
    for (int k = 3; k >= 0; --k) kc = ((plan >> (3 * k)) & 7) == 2 ? k : kc;
    return kc;
}
// does the plan change a pixel at all?
OCN_DEV bool cj_active(int plan) {
    bool on = (plan >> 12) & 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int code = (plan >> (3 * k)) & 7;
        on = on || (code >= 1 && code <= 4);
    }
    return on;
}

OCN_DEV uint64_t cj_wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(CJ_THREADS) void color_jitter_mean_kernel(const uint8_t* img, const float* __restrict__ factors,
                                                                       const int32_t* __restrict__ plan, float* __restrict__ mean_ws, int npix) {
    __shared__ uint64_t part[CJ_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int pl = __builtin_amdgcn_readfirstlane(plan[b]);
    const int kc = cj_first_contrast(pl);
    if (kc == 4) return;
    const float fac[4] = {factors[4 * b], factors[4 * b + 1], factors[4 * b + 2], factors[4 * b + 3]};
    const uint8_t* p = img + (size_t)b * npix * 3;
    const CjSplit s = cj_split((uintptr_t)p, npix);
    uint64_t acc = 0;
    for (int t = tid; t < s.nitems; t += CJ_THREADS) {
        uint32_t w[3];
        float r[4], g[4], bl[4];
        cj_load_item(p, s, t, true, w);
        cj_unpack(w, r, g, bl);
        cj_steps(r, g, bl, pl, fac, 0.f, 0, kc);
        const int n = t < s.ngroups ? 4 : 1;
        uint32_t q = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t qi = (uint32_t)__builtin_rintf(cj_gray(r[i], g[i], bl[i]) * CJ_MEAN_ONE);  // gray <= 0.9999: below 2^24
            q += i < n ? qi : 0u;
        }
        acc += q;
    }
    acc = cj_wave_sum_u64(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        uint64_t total = 0;
#pragma unroll
        for (int i = 0; i < CJ_THREADS / 64; ++i) total += part[i];
        mean_ws[b] = (float)((double)total / ((double)npix * (double)CJ_MEAN_ONE));
    }
}

__global__ __launch_bounds__(CJ_THREADS) void color_jitter_apply_kernel(const uint8_t* img, const float* __restrict__ factors,
                                                                        const int32_t* __restrict__ plan, const float* __restrict__ mean_ws,
                                                                        uint8_t* out, int npix, int nblk) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nblk, j = blockIdx.x - b * nblk;
    const int pl = __builtin_amdgcn_readfirstlane(plan[b]);
    const uint8_t* p = img + (size_t)b * npix * 3;
    uint8_t* o = out + (size_t)b * npix * 3;
    const CjSplit s = cj_split((uintptr_t)o, npix);
    const int t0 = j * CJ_WG_ITEMS;
    const bool active = cj_active(pl);
    if (t0 >= s.nitems || (!active && p == o)) return;  // uniform: past the image's items, or an untouched image in place
    const bool dword = (((uintptr_t)p ^ (uintptr_t)o) & 3) == 0;  // the source's groups are aligned like the destination's
    uint32_t w[CJ_ITEMS][3];
#pragma unroll
    for (int k = 0; k < CJ_ITEMS; ++k) {
        const int t = t0 + k * CJ_THREADS + tid;
        if (t < s.nitems) cj_load_item(p, s, t, dword, w[k]);
    }
    if (active) {  // an image whose plan holds no step and no grayscale is copied as it is: the hue round trip is not exact in fp32
        const float fac[4] = {factors[4 * b], factors[4 * b + 1], factors[4 * b + 2], factors[4 * b + 3]};
        const float m = cj_first_contrast(pl) < 4 ? mean_ws[b] : 0.f;
        const bool gray = (pl >> 12) & 1;
#pragma unroll
        for (int k = 0; k < CJ_ITEMS; ++k) {
            if (t0 + k * CJ_THREADS + tid < s.nitems) {
                float r[4], g[4], bl[4];
                cj_unpack(w[k], r, g, bl);
                cj_steps(r, g, bl, pl, fac, m, 0, 4);
                if (gray) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) r[i] = g[i] = bl[i] = cj_gray(r[i], g[i], bl[i]);
                }
                cj_pack(r, g, bl, w[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CJ_ITEMS; ++k) {
        const int t = t0 + k * CJ_THREADS + tid;
        if (t < s.nitems) cj_store_item(o, s, t, w[k]);
    }
}

}  // namespace

extern "C" int ocn_color_jitter_u8(const void* img_u8, int B, int H, int W, const float* factors, const int32_t* plan, float* mean_ws, void* out_u8,
                                   ocn_stream_t stream) {
    OCN_CHECK_ARG(img_u8 && factors && plan && mean_ws && out_u8, "ocn_color_jitter_u8: null operand");
    OCN_CHECK_ARG((((uintptr_t)factors | (uintptr_t)plan | (uintptr_t)mean_ws) & 3) == 0,
                  "ocn_color_jitter_u8: factors, plan and mean_ws must be 4-byte aligned");
    OCN_CHECK_ARG(B > 0 && H >= 1 && H <= CJ_MAX_SIDE && W >= 1 && W <= CJ_MAX_SIDE,
                  "ocn_color_jitter_u8: bad shape B=%d H=%d W=%d (B >= 1, 1 <= H, W <= %d)", B, H, W, CJ_MAX_SIDE);
    const int npix = H * W;
    const int nblk = ocn_cdiv(npix / 4 + 6, CJ_WG_ITEMS);  // an image has at most npix / 4 + 6 items (3 head and 3 tail pixels)
    const long nwg = (long)B * nblk;
    OCN_CHECK_ARG(nwg <= 0x7fffffffL, "ocn_color_jitter_u8: B=%d images of %d workgroups exceed the grid", B, nblk);
    hipLaunchKernelGGL(color_jitter_mean_kernel, dim3((unsigned)B), dim3(CJ_THREADS), 0, (hipStream_t)stream, (const uint8_t*)img_u8, factors, plan,
                       mean_ws, npix);
    OCN_CHECK_LAUNCH("ocn_color_jitter_u8 (mean)");
    hipLaunchKernelGGL(color_jitter_apply_kernel, dim3((unsigned)nwg), dim3(CJ_THREADS), 0, (hipStream_t)stream, (const uint8_t*)img_u8, factors, plan,
                       mean_ws, (uint8_t*)out_u8, npix, nblk);
    OCN_CHECK_LAUNCH("ocn_color_jitter_u8 (apply)");
    return OCN_OK;
}
