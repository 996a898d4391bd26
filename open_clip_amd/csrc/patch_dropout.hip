// Patch dropout of the image tower (reference transformer.py:17-58 `PatchDropout`, applied at :804 after the class token and the positional
// embedding): which patches survive does not depend on their values, so the native path chooses them FIRST (patch_keep_plan_kernel) and
// patchifies, multiplies and assembles only the K kept patches of every image.  This file only decides WHICH patches survive (the plan and its
// inverse); everything that is done with `keep` / `inv` is in embed.hip.
#include "ocn_common.h"

namespace {

constexpr int PLAN_MAX_G = 4096;

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), written out: counter (c0..c3), key (k0, k1); word 0 of the
// result.  Counter-based: the key of patch g of image b depends on (seed, b, g) alone, never on the launch geometry.
OCN_DEV uint32_t philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// One workgroup per image: a 32-bit key per patch in LDS, patch g is kept iff fewer than K patches rank before it (larger key first, equal keys by
// index: a strict total order, so exactly K survive) -- the K-subset `randn(B, G).topk(K)` draws (transformer.py:50-51), uniform over all subsets.
// keep[b, :] = the kept indices ASCENDING (their position = a prefix count over the kept flags), inv[b, g] = that position or -1.
__global__ __launch_bounds__(256) void patch_keep_plan_kernel(uint32_t seed_lo, uint32_t seed_hi, int G, int K, int32_t* __restrict__ keep,
                                                              int32_t* __restrict__ inv) {
    __shared__ __attribute__((aligned(16))) uint32_t keys[PLAN_MAX_G];
    __shared__ int wcnt[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int G4 = (G + 3) & ~3;  // padding keys are 0 at an index >= G: they rank before nothing
    for (int g = tid; g < G4; g += 256) keys[g] = g < G ? philox4x32_10((uint32_t)g, (uint32_t)b, 0u, 0u, seed_lo, seed_hi) : 0u;
    __syncthreads();
    int carry = 0;  // kept patches in front of this chunk (the same value in every thread)
    for (int base = 0; base < G; base += 256) {
        const int g = base + tid;
        bool kept = false;
        if (g < G) {
            const uint32_t kg = keys[g];
            int rank = 0;
            for (int h = 0; h < G4; h += 4) {  // every lane reads the same 16 bytes: an LDS broadcast
                const uint4 kh = *(const uint4*)(keys + h);
                rank += (kh.x > kg || (kh.x == kg && h < g)) ? 1 : 0;
                rank += (kh.y > kg || (kh.y == kg && h + 1 < g)) ? 1 : 0;
                rank += (kh.z > kg || (kh.z == kg && h + 2 < g)) ? 1 : 0;
                rank += (kh.w > kg || (kh.w == kg && h + 3 < g)) ? 1 : 0;
            }
            kept = rank < K;
        }
        const unsigned long long m = __ballot(kept);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int pre = carry, tot = 0;
        for (int k = 0; k < 4; ++k) {
            if (k < w) pre += wcnt[k];
            tot += wcnt[k];
        }
        const int j = pre + __popcll(m & ((1ull << lane) - 1ull));
        if (g < G) inv[(size_t)b * G + g] = kept ? j : -1;
        if (kept) keep[(size_t)b * K + j] = g;
        carry += tot;
        __syncthreads();  // wcnt is rewritten by the next chunk
    }
}

// inv of a caller-supplied keep (any order; distinct indices): inv[b, keep[b, j]] = j, -1 elsewhere.  One workgroup per image.
__global__ __launch_bounds__(256) void patch_keep_inverse_kernel(const int32_t* __restrict__ keep, int32_t* __restrict__ inv, int G, int K) {
    const int b = blockIdx.x;
    for (int g = threadIdx.x; g < G; g += 256) inv[(size_t)b * G + g] = -1;
    __syncthreads();
    for (int j = threadIdx.x; j < K; j += 256) {
        const int g = keep[(size_t)b * K + j];
        inv[(size_t)b * G + ocn_clamp_index(g, G)] = j;
    }
}

}  // namespace

extern "C" int ocn_patch_keep_plan(int64_t seed, int B, int G, int K, int32_t* keep, int32_t* inv, ocn_stream_t stream) {
    OCN_CHECK_ARG(keep && inv, "ocn_patch_keep_plan: null operand");
    OCN_CHECK_ARG(B > 0 && G > 0 && G <= PLAN_MAX_G && K > 0 && K <= G, "ocn_patch_keep_plan: bad shape B=%d G=%d K=%d (1 <= K <= G <= %d)", B, G, K,
                  PLAN_MAX_G);
    hipLaunchKernelGGL(patch_keep_plan_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32), G, K, keep, inv);
    OCN_CHECK_LAUNCH("ocn_patch_keep_plan");
    return OCN_OK;
}

extern "C" int ocn_patch_keep_inverse(const int32_t* keep, int32_t* inv, int B, int G, int K, ocn_stream_t stream) {
    OCN_CHECK_ARG(keep && inv, "ocn_patch_keep_inverse: null operand");
    OCN_CHECK_ARG(B > 0 && G > 0 && K > 0 && K <= G, "ocn_patch_keep_inverse: bad shape B=%d G=%d K=%d (1 <= K <= G)", B, G, K);
    hipLaunchKernelGGL(patch_keep_inverse_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, keep, inv, G, K);
    OCN_CHECK_LAUNCH("ocn_patch_keep_inverse");
    return OCN_OK;
}
