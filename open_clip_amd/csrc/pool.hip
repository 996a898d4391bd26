// Mean pooling over the tokens of an image (`pool_type = "avg"`: x[:, 1:].mean(dim=1), transformer.py:783-785), its backward, and the widening
// cast bf16 -> fp32.  All three are HBM-bound streams: wave64, 16 bytes per lane and access, no atomics, one fixed order of additions -- the same bits
// in every run, so `deterministic` needs no second form.
#include "ocn_common.h"

namespace {

constexpr int POOL_WAVES = 8;      // waves of a forward workgroup: the token range of one image is dealt out over them
constexpr int POOL_BWD_ROWS = 32;  // token rows one backward workgroup writes (4 waves, 8 rows each; 16 / 32 rows measured alike, 64 and more slower)

// One workgroup = one image x one slab of 64 * VEC columns (VEC = 16 bytes of x per lane); grid: image * slabs + slab.  Wave w adds the tokens skip + w, skip + w + 8, ... in
// that order into fp32 registers; the eight partial sums meet in LDS and wave 0 adds them in wave order, then divides ONCE (correctly rounded).
template <bool X16>
__global__ __launch_bounds__(POOL_WAVES * 64) void mean_pool_fwd_kernel(const void* __restrict__ xv, float* __restrict__ out, int T, int skip, int C,
                                                                        int slabs) {
    constexpr int VEC = X16 ? 8 : 4;
    __shared__ float part[POOL_WAVES][VEC][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the slab is the fastest index of the grid: workgroups that run together read WHOLE rows between them (with the image fastest, all of them read
    // the same 1 KiB of every row at a time, which lands on a part of the memory channels only: 2.6 instead of 5 TB/s measured)
    const int b = blockIdx.x / slabs;
    const int col = ((blockIdx.x - b * slabs) * 64 + lane) * VEC;
    const bool live = col < C;  // C % 8 == 0: the VEC columns of a lane lie inside the row or outside it as a whole
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    if (live) {
        const size_t row0 = (size_t)b * T;
#pragma unroll 4
        for (int t = skip + wave; t < T; t += POOL_WAVES) {
            const size_t off = (row0 + t) * (size_t)C + col;
            if (X16) {
                const bf16x8 v = *(const bf16x8*)((const bf16*)xv + off);
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] += bf2f(v[i]);
            } else {
                const f32x4 v = *(const f32x4*)((const float*)xv + off);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += v[i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) part[wave][i][lane] = acc[i];
    __syncthreads();
    if (wave == 0 && live) {
        const float n = (float)(T - skip);
        float s[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s[i] = part[0][i][lane];
#pragma unroll
            for (int w = 1; w < POOL_WAVES; ++w) s[i] += part[w][i][lane];
            s[i] = __fdiv_rn(s[i], n);
        }
        float* o = out + (size_t)b * C + col;
#pragma unroll
        for (int i = 0; i < VEC; i += 4) *(f32x4*)(o + i) = (f32x4){s[i], s[i + 1], s[i + 2], s[i + 3]};
    }
}

// One workgroup = one image x POOL_BWD_ROWS token rows x one slab of 512 columns.  Every row t >= skip of an image is the same vector dpooled[b] / n,
// so each lane forms its 16-byte pieces once -- two fp32 pieces (columns 4 * lane and 256 + 4 * lane of the slab: a wave's store covers 1 KiB without
// a gap) and one bf16 piece (columns 8 * lane) -- and then only stores; rows t < skip receive zeros from the same stores.
__global__ __launch_bounds__(256) void mean_pool_bwd_kernel(const float* __restrict__ dp, float* __restrict__ dx, bf16* __restrict__ dx16, int T, int skip,
                                                            int C, int slabs, int chunks) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int piece = blockIdx.x / slabs;  // slab fastest, as in the forward: neighbouring workgroups write whole rows between them
    const int slab = (blockIdx.x - piece * slabs) * 512;
    const int b = piece / chunks, chunk = piece - b * chunks;
    const int ca = slab + 4 * lane, cb = ca + 256, c8 = slab + 8 * lane;
    const bool la = dx != nullptr && ca < C, lb = dx != nullptr && cb < C, l8 = dx16 != nullptr && c8 < C;
    const float n = (float)(T - skip);
    const float* d = dp + (size_t)b * C;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 va = zero, vb = zero;
    bf16x8 v8, z8;
#pragma unroll
    for (int i = 0; i < 8; ++i) v8[i] = z8[i] = f2bf(0.f);
    if (la) {
        va = *(const f32x4*)(d + ca);
#pragma unroll
        for (int i = 0; i < 4; ++i) va[i] = __fdiv_rn(va[i], n);
    }
    if (lb) {
        vb = *(const f32x4*)(d + cb);
#pragma unroll
        for (int i = 0; i < 4; ++i) vb[i] = __fdiv_rn(vb[i], n);
    }
    if (l8) {
        const f32x4 lo = *(const f32x4*)(d + c8), hi = *(const f32x4*)(d + c8 + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v8[i] = f2bf(__fdiv_rn(lo[i], n));
            v8[4 + i] = f2bf(__fdiv_rn(hi[i], n));
        }
    }
    const int t0 = chunk * POOL_BWD_ROWS;
    const int t1 = t0 + POOL_BWD_ROWS < T ? t0 + POOL_BWD_ROWS : T;
    for (int t = t0 + wave; t < t1; t += 4) {
        const bool z = t < skip;
        const size_t r = ((size_t)b * T + t) * (size_t)C;
        if (la) *(f32x4*)(dx + r + ca) = z ? zero : va;
        if (lb) *(f32x4*)(dx + r + cb) = z ? zero : vb;
        if (l8) *(bf16x8*)(dx16 + r + c8) = z ? z8 : v8;
    }
}

// dst fp32 = src bf16, exact: 8 elements (16 bytes in, 2 x 16 bytes out) per lane and step, the last n % 8 elements one by one
__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(const bf16* __restrict__ src, float* __restrict__ dst, long n) {
    const long n8 = n >> 3;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const bf16x8 v = *(const bf16x8*)(src + i * 8);
        *(f32x4*)(dst + i * 8) = (f32x4){bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])};
        *(f32x4*)(dst + i * 8 + 4) = (f32x4){bf2f(v[4]), bf2f(v[5]), bf2f(v[6]), bf2f(v[7])};
    }
    if (blockIdx.x == 0) {
        const long k = n8 * 8 + threadIdx.x;
        if (threadIdx.x < 8 && k < n) dst[k] = bf2f(src[k]);
    }
}

bool pool_args_ok(const char* name, const void* a, const void* b, int B, int T, int skip, int C) {
    if (!a || !b) {
        ocn_set_error("%s: null operand", name);
        return false;
    }
    if (B <= 0 || C <= 0) {
        ocn_set_error("%s: B=%d and C=%d must be positive", name, B, C);
        return false;
    }
    if (skip < 0 || skip >= T) {
        ocn_set_error("%s: skip=%d must satisfy 0 <= skip < T=%d", name, skip, T);
        return false;
    }
    if (C % 8 != 0) {
        ocn_set_error("%s: C=%d must be a multiple of 8", name, C);
        return false;
    }
    if ((long)B * T > 0x7fffffffL) {
        ocn_set_error("%s: B*T=%ld rows exceed the int32 range", name, (long)B * T);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int ocn_mean_pool_fwd(const void* x, int x_is_bf16, float* out, int B, int T, int skip, int C, ocn_stream_t stream) {
    if (!pool_args_ok("ocn_mean_pool_fwd", x, out, B, T, skip, C)) return OCN_ERR_INVALID;
    OCN_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0, "ocn_mean_pool_fwd: operands must be 16-byte aligned");
    const int per_slab = 64 * (x_is_bf16 ? 8 : 4);
    const int slabs = ocn_cdiv(C, per_slab);
    OCN_CHECK_ARG((long)B * slabs <= 0x7fffffffL, "ocn_mean_pool_fwd: B=%d x C=%d too large for one launch", B, C);
    const dim3 grid(B * slabs), block(POOL_WAVES * 64);
    if (x_is_bf16)
        hipLaunchKernelGGL(mean_pool_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, x, out, T, skip, C, slabs);
    else
        hipLaunchKernelGGL(mean_pool_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, x, out, T, skip, C, slabs);
    OCN_CHECK_LAUNCH("ocn_mean_pool_fwd");
    return OCN_OK;
}

extern "C" int ocn_mean_pool_bwd(const float* dpooled, float* dx, void* dx_bf16, int B, int T, int skip, int C, ocn_stream_t stream) {
    if (!pool_args_ok("ocn_mean_pool_bwd", dpooled, dx ? (void*)dx : dx_bf16, B, T, skip, C)) return OCN_ERR_INVALID;
    OCN_CHECK_ARG(((uintptr_t)dpooled & 15) == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)dx_bf16 & 15) == 0,
                  "ocn_mean_pool_bwd: operands must be 16-byte aligned");
    const int chunks = ocn_cdiv(T, POOL_BWD_ROWS), slabs = ocn_cdiv(C, 512);
    OCN_CHECK_ARG((long)B * chunks * slabs <= 0x7fffffffL, "ocn_mean_pool_bwd: B=%d x T=%d x C=%d too large for one launch", B, T, C);
    hipLaunchKernelGGL(mean_pool_bwd_kernel, dim3(B * chunks * slabs), dim3(256), 0, (hipStream_t)stream, dpooled, dx, (bf16*)dx_bf16, T, skip, C, slabs,
                       chunks);
    OCN_CHECK_LAUNCH("ocn_mean_pool_bwd");
    return OCN_OK;
}

extern "C" int ocn_cast_bf16_f32(const void* src, float* dst, int64_t n, ocn_stream_t stream) {
    OCN_CHECK_ARG(src && dst, "ocn_cast_bf16_f32: null operand");
    OCN_CHECK_ARG(n > 0, "ocn_cast_bf16_f32: n=%ld must be positive", (long)n);
    OCN_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "ocn_cast_bf16_f32: operands must be 16-byte aligned");
    hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(ocn_grid_for((n + 7) / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)src, dst, (long)n);
    OCN_CHECK_LAUNCH("ocn_cast_bf16_f32");
    return OCN_OK;
}
