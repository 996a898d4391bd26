// Weight casts (fp32 master -> bf16 operand copies), grad-norm and AdamW (HBM-bound elementwise kernels).
#include "ocn_common.h"

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include <cmath>

namespace {

__global__ void cast_kernel(const float* __restrict__ src, bf16* __restrict__ dst, long n) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 v = *(const f32x4*)(src + i * 4);
        bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
        *(bf16x4*)(dst + i * 4) = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[n4 * 4 + threadIdx.x] = f2bf(src[n4 * 4 + threadIdx.x]);
}

// dst = bf16(src * *scale): the scale stays on the device (logit_scale.exp() of the loss, loss.py:103-110 `logit_scale * image_features`)
__global__ void cast_scaled_kernel(const float* __restrict__ src, bf16* __restrict__ dst, long n, const float* __restrict__ scale) {
    const float s = *scale;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 v = *(const f32x4*)(src + i * 4);
        bf16x4 o = {f2bf(v[0] * s), f2bf(v[1] * s), f2bf(v[2] * s), f2bf(v[3] * s)};
        *(bf16x4*)(dst + i * 4) = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[n4 * 4 + threadIdx.x] = f2bf(src[n4 * 4 + threadIdx.x] * s);
}

// dst[C,R] = src[R,C]^T, 64x64 tiles through LDS (both sides coalesced)
__global__ __launch_bounds__(256) void cast_transpose_kernel(const float* __restrict__ src, bf16* __restrict__ dst, int R, int C) {
    __shared__ float tile[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < R && c < C) ? src[(size_t)r * C + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < C && r < R) dst[(size_t)c * R + r] = f2bf(tile[tx][i]);
    }
}

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, long n, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 v = *(const f32x4*)(x + i * 4);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float v = x[n4 * 4 + threadIdx.x];
        s += v * v;
    }
    const float t = block_sum_256(s, red);
    if (threadIdx.x == 0) unsafeAtomicAdd(out, t);
}

// torch.optim.AdamW (single-tensor form): p *= 1 - lr*wd; m,v EMA; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
__global__ void adamw_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             bf16* __restrict__ w16, long n, float lr, float b1, float b2, float eps, float wd, float bc1,
                             float bc2_sqrt, const float* __restrict__ clip_coef) {
    const float gs = clip_coef ? *clip_coef : 1.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float gi = g[i] * gs;
        float p = w[i] * (1.0f - lr * wd);
        const float mi = m[i] + (gi - m[i]) * (1.0f - b1);          // lerp form used by torch
        const float vi = v[i] * b2 + gi * gi * (1.0f - b2);
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p -= (lr / bc1) * (mi / denom);
        w[i] = p;
        m[i] = mi;
        v[i] = vi;
        if (w16) w16[i] = f2bf(p);
    }
}


// ---- whole-model optimizer step in ONE launch --------------------------------------------------------
// The host describes every tensor by an AdamEntry and cuts the work into chunks {entry, index}: a chunk is 8192 consecutive
// elements (mode 0: 16-byte vector path, mode 2: scalar path for odd sizes / alignments) or one 64x64 tile of a 2-D GEMM
// weight (mode 1).  Besides torch.optim.AdamW's update the kernel refreshes the bf16 operand copies of the GEMM weights in
// the same pass -- the plain copy [rows, cols] and, in tile mode, the transposed copy [cols, rows] through LDS -- and applies
// the clip_grad_norm_ coefficient (grad_clip_coef, ocn_common.h) of the squared gradient norm that ocn_sumsq_multi left on the device.
struct AdamEntry {
    float* w;
    const float* g;
    float* m;
    float* v;
    bf16* w16n;
    bf16* w16t;
    long numel;
    int rows, cols, mode, pad;
    // the four per-step floats, by update rule:  AdamW | NAdamW (nadam_one)
    union { float lr; float decay; };      // lr                      | 1 - lr * wd
    union { float wd; float bc2; };        // weight decay            | 1 - beta2^step
    union { float bc1; float c_g; };       // 1 - beta1^step          | lr (1 - mu_t) / (1 - mu_product)
    union { float bc2_sqrt; float c_m; };  // sqrt(1 - beta2^step)    | lr mu_next / (1 - mu_product mu_next)
};
static_assert(sizeof(AdamEntry) == 88, "AdamEntry layout is mirrored by open_clip_amd/tables.py");
constexpr int ADAM_CHUNK = 8192;

// omb1 / omb2: 1 - beta1 / 1 - beta2 as the entry point hands them over (ocn_adamw_multi: the fp32 differences; ocn_nadamw_multi: the caller's)
OCN_DEV float adam_one(float w, float gi, float& m, float& v, float lr, float wd, float omb1, float b2, float omb2, float eps, float bc1, float bc2_sqrt) {
    float p = w * (1.0f - lr * wd);
    m = m + (gi - m) * omb1;
    v = v * b2 + gi * gi * omb2;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    return p - (lr / bc1) * (m / denom);
}

// torch.optim.NAdam(decoupled_weight_decay=True), single-tensor form: the momentum schedule (mu_t, mu_next, mu_product) is host state, the record
// carries what it leaves for the element:  p *= decay; m, v EMA; den = sqrt(v / bc2) + eps; p -= c_g * g / den; p -= c_m * m / den
OCN_DEV float nadam_one(float w, float gi, float& m, float& v, float decay, float omb1, float b2, float omb2, float eps, float bc2, float c_g, float c_m) {
    float p = w * decay;
    m = m + (gi - m) * omb1;
    v = v * b2 + gi * gi * omb2;
    const float denom = sqrtf(v / bc2) + eps;
    p -= c_g * (gi / denom);
    return p - c_m * (m / denom);
}

enum { RULE_ADAMW = 0, RULE_NADAMW = 1 };

template <int RULE>
OCN_DEV float update_one(const AdamEntry& e, float w, float gi, float& m, float& v, float omb1, float b2, float omb2, float eps) {
    if constexpr (RULE == RULE_NADAMW) return nadam_one(w, gi, m, v, e.decay, omb1, b2, omb2, eps, e.bc2, e.c_g, e.c_m);
    else return adam_one(w, gi, m, v, e.lr, e.wd, omb1, b2, omb2, eps, e.bc1, e.bc2_sqrt);
}

// the walk of one {numel, index, mode} chunk outside tile mode: ADAM_CHUNK consecutive elements per workgroup of 256 threads.  Mode 0: quad(i) on
// 16-byte vectors, i = base + 4 t, + 1024, ..., then one(i) on the numel % 4 leftovers of the last chunk; any other mode: one(i), i = base + t, + 256, ...
template <typename Quad, typename One>
OCN_DEV void chunk_walk(long numel, int index, int mode, Quad quad, One one) {
    const long base = (long)index * ADAM_CHUNK;
    const long end = base + ADAM_CHUNK < numel ? base + ADAM_CHUNK : numel;
    if (mode == 0) {
        for (long i = base + threadIdx.x * 4; i + 3 < end; i += 1024) quad(i);
        const long tail = end - ((end - base) & 3);
        if (tail + threadIdx.x < end) one(tail + threadIdx.x);
    } else {
        for (long i = base + threadIdx.x; i < end; i += 256) one(i);
    }
}

// one element: load, update, store w, m, v and the plain bf16 copy -- the numel % 4 leftovers of the vector path and the whole scalar path
template <int RULE>
OCN_DEV void adam_single(const AdamEntry& e, long i, float gs, float omb1, float b2, float omb2, float eps) {
    float mi = e.m[i], vi = e.v[i];
    const float p = update_one<RULE>(e, e.w[i], e.g[i] * gs, mi, vi, omb1, b2, omb2, eps);
    e.w[i] = p; e.m[i] = mi; e.v[i] = vi;
    if (e.w16n) e.w16n[i] = f2bf(p);
}

// one walk over the chunk table for every update rule: RULE picks the element update, everything else (modes, operand copies, clip) is shared.
// The two four-element loops (tile mode, vector path) and the walk of modes 0 / 2 stay written out in the kernel body: behind adam_quad / chunk_walk
// (as a function or as a lambda) the compiler pairs the lanes of  v * b2 + g * g * omb2  the other way round in the vector path and contracts the
// other product into the FMA -- exp_avg_sq moves by an ulp in a quarter of the elements (tests/test_optim_parent_gpu.py).
template <int RULE>
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamEntry* __restrict__ entries, const int2* __restrict__ chunks,
                                                         float omb1, float b2, float omb2, float eps, const float* __restrict__ gnorm_sq,
                                                         float max_norm) {
    __shared__ float tile[64][65];
    const int2 ch = chunks[blockIdx.x];
    const AdamEntry e = entries[ch.x];
    const float gs = grad_clip_coef(gnorm_sq, max_norm);
    if (e.mode == 1) {
        const int tiles_c = e.cols >> 6;
        const int r0 = (ch.y / tiles_c) * 64, c0 = (ch.y % tiles_c) * 64;
        const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
        const bool g_vec = ((uintptr_t)e.g & 15) == 0;  // gradients may be views into a DDP bucket at any 4-byte offset
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = ty + 16 * k;
            const size_t o = (size_t)(r0 + r) * e.cols + c0 + tx * 4;
            const f32x4 g4 = g_vec ? *(const f32x4*)(e.g + o) : (f32x4){e.g[o], e.g[o + 1], e.g[o + 2], e.g[o + 3]};
            const f32x4 w4 = *(const f32x4*)(e.w + o);
            f32x4 m4 = *(const f32x4*)(e.m + o), v4 = *(const f32x4*)(e.v + o), p4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float mj = m4[j], vj = v4[j];
                p4[j] = update_one<RULE>(e, w4[j], g4[j] * gs, mj, vj, omb1, b2, omb2, eps);
                m4[j] = mj;
                v4[j] = vj;
            }
            *(f32x4*)(e.w + o) = p4;
            *(f32x4*)(e.m + o) = m4;
            *(f32x4*)(e.v + o) = v4;
            if (e.w16n) *(bf16x4*)(e.w16n + o) = (bf16x4){f2bf(p4[0]), f2bf(p4[1]), f2bf(p4[2]), f2bf(p4[3])};
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[r][tx * 4 + j] = p4[j];
        }
        if (e.w16t) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = ty + 16 * k;  // row of the transposed copy
                const bf16x4 o4 = {f2bf(tile[tx * 4][c]), f2bf(tile[tx * 4 + 1][c]), f2bf(tile[tx * 4 + 2][c]), f2bf(tile[tx * 4 + 3][c])};
                *(bf16x4*)(e.w16t + (size_t)(c0 + c) * e.rows + r0 + tx * 4) = o4;
            }
        }
        return;
    }
    const long base = (long)ch.y * ADAM_CHUNK;
    const long end = base + ADAM_CHUNK < e.numel ? base + ADAM_CHUNK : e.numel;
    if (e.mode == 0) {
        for (long i = base + threadIdx.x * 4; i + 3 < end; i += 1024) {
            const f32x4 g4 = *(const f32x4*)(e.g + i), w4 = *(const f32x4*)(e.w + i);
            f32x4 m4 = *(const f32x4*)(e.m + i), v4 = *(const f32x4*)(e.v + i), p4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float mj = m4[j], vj = v4[j];
                p4[j] = update_one<RULE>(e, w4[j], g4[j] * gs, mj, vj, omb1, b2, omb2, eps);
                m4[j] = mj;
                v4[j] = vj;
            }
            *(f32x4*)(e.w + i) = p4;
            *(f32x4*)(e.m + i) = m4;
            *(f32x4*)(e.v + i) = v4;
            if (e.w16n) *(bf16x4*)(e.w16n + i) = (bf16x4){f2bf(p4[0]), f2bf(p4[1]), f2bf(p4[2]), f2bf(p4[3])};
        }
        const long tail = end - ((end - base) & 3);  // numel % 4 leftovers of the last chunk
        if (tail + threadIdx.x < end) adam_single<RULE>(e, tail + threadIdx.x, gs, omb1, b2, omb2, eps);
    } else {
        for (long i = base + threadIdx.x; i < end; i += 256) adam_single<RULE>(e, i, gs, omb1, b2, omb2, eps);
    }
}

// out[0] += sum over every tensor of g^2 (same entry / chunk tables as adam_multi_kernel)
// chunk_ws != nullptr: the reproducible form -- the chunk's partial is stored to its own slot, sumsq_fold_kernel adds the slots in order
__global__ __launch_bounds__(256) void sumsq_multi_kernel(const AdamEntry* __restrict__ entries, const int2* __restrict__ chunks,
                                                          float* __restrict__ out, float* __restrict__ chunk_ws) {
    __shared__ float red[4];
    const int2 ch = chunks[blockIdx.x];
    const AdamEntry e = entries[ch.x];
    float s = 0.f;
    if (e.mode == 1) {
        const int tiles_c = e.cols >> 6;
        const int r0 = (ch.y / tiles_c) * 64, c0 = (ch.y % tiles_c) * 64;
        const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* gp = e.g + (size_t)(r0 + ty + 16 * k) * e.cols + c0 + tx * 4;
            s += gp[0] * gp[0] + gp[1] * gp[1] + gp[2] * gp[2] + gp[3] * gp[3];
        }
    } else {
        const long base = (long)ch.y * ADAM_CHUNK;
        const long end = base + ADAM_CHUNK < e.numel ? base + ADAM_CHUNK : e.numel;
        for (long i = base + threadIdx.x; i < end; i += 256) s += e.g[i] * e.g[i];  // this order is what the fixed-order norm's bits are made of
    }
    const float t = block_sum_256(s, red);
    if (threadIdx.x == 0) {
        if (chunk_ws) chunk_ws[blockIdx.x] = t; else unsafeAtomicAdd(out, t);
    }
}

// out[0] += sum of ws[0 .. n) in ONE fixed order: thread t adds ws[t], ws[t + 256], ... ; the 256 partials fold through the wave butterflies and
// four LDS slots (the same additions in the same order in every run)
__global__ __launch_bounds__(256) void sumsq_fold_kernel(const float* __restrict__ ws, int n, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += ws[i];
    const float t = block_sum_256(s, red);
    if (threadIdx.x == 0) out[0] += t;
}

// ---- model EMA: the weight average of the whole model in ONE launch (open_clip_amd/ema.py::NativeModelEma) -----------------------------------
// chunk_walk (8192 consecutive elements per workgroup; mode 0: 16-byte vectors, mode 2: scalar for a pointer off the 16-byte grid) over two
// pointers per tensor.  Pure streaming: 8 B read + 4 B written per element, no LDS, no atomics.
struct EmaEntry {
    float* ema;
    const float* src;
    long numel;
    int mode, pad;
};
static_assert(sizeof(EmaEntry) == 32, "EmaEntry layout is mirrored by open_clip_amd/ema.py");

// torch.lerp's two-branch form: both limits are exact (weight 0 leaves e, weight 1 gives s, bit for bit)
OCN_DEV float ema_one(float e, float s, float weight, float omw) {
    const float d = s - e;
    return weight < 0.5f ? e + weight * d : s - d * omw;
}

__global__ __launch_bounds__(256) void ema_lerp_multi_kernel(const EmaEntry* __restrict__ entries, const int2* __restrict__ chunks, float weight,
                                                             float omw) {
    const int2 ch = chunks[blockIdx.x];
    const EmaEntry e = entries[ch.x];
    chunk_walk(e.numel, ch.y, e.mode,
               [&](long i) {
                   f32x4 a4 = *(const f32x4*)(e.ema + i);
                   const f32x4 s4 = *(const f32x4*)(e.src + i);
#pragma unroll
                   for (int j = 0; j < 4; ++j) a4[j] = ema_one(a4[j], s4[j], weight, omw);
                   *(f32x4*)(e.ema + i) = a4;
               },
               [&](long i) { e.ema[i] = ema_one(e.ema[i], e.src[i], weight, omw); });
}

// workgroups of a grid-stride launch in this file: at most 4096 (ocn_grid_for's cap is 8192)
int grid_for_4096(long items, int block) {
    long g = (items + block - 1) / block;
    return (int)(g < 4096 ? (g > 0 ? g : 1) : 4096);
}

}  // namespace

extern "C" int ocn_cast_f32_bf16(const float* src, void* dst, int64_t n, ocn_stream_t stream) {
    OCN_CHECK_ARG(src && dst && n > 0, "ocn_cast_f32_bf16: bad arguments");
    OCN_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 7) == 0, "ocn_cast_f32_bf16: misaligned");
    hipLaunchKernelGGL(cast_kernel, dim3(grid_for_4096((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, (long)n);
    OCN_CHECK_LAUNCH("ocn_cast_f32_bf16");
    return OCN_OK;
}

extern "C" int ocn_cast_f32_bf16_scaled(const float* src, void* dst, int64_t n, const float* scale_dev, ocn_stream_t stream) {
    OCN_CHECK_ARG(src && dst && n > 0 && scale_dev, "ocn_cast_f32_bf16_scaled: bad arguments");
    OCN_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 7) == 0, "ocn_cast_f32_bf16_scaled: misaligned");
    hipLaunchKernelGGL(cast_scaled_kernel, dim3(grid_for_4096((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, (long)n, scale_dev);
    OCN_CHECK_LAUNCH("ocn_cast_f32_bf16_scaled");
    return OCN_OK;
}

extern "C" int ocn_cast_transpose_f32_bf16(const float* src, void* dst, int R, int C, ocn_stream_t stream) {
    OCN_CHECK_ARG(src && dst && R > 0 && C > 0, "ocn_cast_transpose_f32_bf16: bad arguments");
    hipLaunchKernelGGL(cast_transpose_kernel, dim3(ocn_cdiv(C, 64), ocn_cdiv(R, 64)), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, R, C);
    OCN_CHECK_LAUNCH("ocn_cast_transpose_f32_bf16");
    return OCN_OK;
}

extern "C" int ocn_sumsq_accum(const float* x, int64_t n, float* out, ocn_stream_t stream) {
    OCN_CHECK_ARG(x && out && n > 0, "ocn_sumsq_accum: bad arguments");
    OCN_CHECK_ARG(((uintptr_t)x & 15) == 0, "ocn_sumsq_accum: misaligned");
    int g = grid_for_4096((n + 3) / 4, 256);
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(sumsq_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, x, (long)n, out);
    OCN_CHECK_LAUNCH("ocn_sumsq_accum");
    return OCN_OK;
}

extern "C" int ocn_adamw_step(float* w, const float* g, float* m, float* v, void* w_bf16, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, const float* clip_coef,
                              ocn_stream_t stream) {
    OCN_CHECK_ARG(w && g && m && v && n > 0 && step >= 1, "ocn_adamw_step: bad arguments");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_for_4096(n, 256)), dim3(256), 0, (hipStream_t)stream, w, g, m, v, (bf16*)w_bf16, (long)n,
                       lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, clip_coef);
    OCN_CHECK_LAUNCH("ocn_adamw_step");
    return OCN_OK;
}

extern "C" int ocn_adamw_multi(const void* entries, const void* chunks, int n_chunks, float beta1, float beta2, float eps,
                               const float* gnorm_sq, float max_norm, ocn_stream_t stream) {
    OCN_CHECK_ARG(entries && chunks && n_chunks > 0, "ocn_adamw_multi: bad arguments");
    hipLaunchKernelGGL(adam_multi_kernel<RULE_ADAMW>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamEntry*)entries,
                       (const int2*)chunks, 1.0f - beta1, beta2, 1.0f - beta2, eps, gnorm_sq, max_norm);
    OCN_CHECK_LAUNCH("ocn_adamw_multi");
    return OCN_OK;
}

extern "C" int ocn_nadamw_multi(const void* entries, const void* chunks, int n_chunks, float one_minus_beta1, float beta2, float one_minus_beta2,
                                float eps, const float* gnorm_sq, float max_norm, ocn_stream_t stream) {
    OCN_CHECK_ARG(entries && chunks, "ocn_nadamw_multi: null entry / chunk table");
    OCN_CHECK_ARG(n_chunks > 0, "ocn_nadamw_multi: n_chunks must be positive");
    hipLaunchKernelGGL(adam_multi_kernel<RULE_NADAMW>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamEntry*)entries,
                       (const int2*)chunks, one_minus_beta1, beta2, one_minus_beta2, eps, gnorm_sq, max_norm);
    OCN_CHECK_LAUNCH("ocn_nadamw_multi");
    return OCN_OK;
}

extern "C" int ocn_sumsq_multi(const void* entries, const void* chunks, int n_chunks, float* out, float* chunk_ws, ocn_stream_t stream) {
    OCN_CHECK_ARG(entries && chunks && out && n_chunks > 0, "ocn_sumsq_multi: bad arguments");
    hipLaunchKernelGGL(sumsq_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AdamEntry*)entries,
                       (const int2*)chunks, out, chunk_ws);
    OCN_CHECK_LAUNCH("ocn_sumsq_multi");
    if (chunk_ws) {
        hipLaunchKernelGGL(sumsq_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, chunk_ws, n_chunks, out);
        OCN_CHECK_LAUNCH("ocn_sumsq_multi (fold)");
    }
    return OCN_OK;
}

extern "C" int ocn_ema_lerp_multi(const void* entries, const void* chunks, int n_chunks, float weight, ocn_stream_t stream) {
    OCN_CHECK_ARG(entries && chunks, "ocn_ema_lerp_multi: null entry / chunk table");
    OCN_CHECK_ARG(n_chunks >= 0, "ocn_ema_lerp_multi: n_chunks must not be negative");
    OCN_CHECK_ARG(std::isfinite(weight), "ocn_ema_lerp_multi: weight must be finite");
    if (n_chunks == 0) return OCN_OK;
    hipLaunchKernelGGL(ema_lerp_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const EmaEntry*)entries, (const int2*)chunks,
                       weight, 1.0f - weight);
    OCN_CHECK_LAUNCH("ocn_ema_lerp_multi");
    return OCN_OK;
}
