// Validation metrics: the rank of every query's labelled candidate among all candidates (open_clip_train/metrics.py:95-169 `_paired_retrieval_ranks`,
// open_clip_train/zero_shot.py:15-18 `accuracy`) without a score matrix in memory, and the operand preparation of its fp32 mode.
//
// One tile routine computes every score: a workgroup of 4 waves forms a 256 (candidates) x 128 (queries) tile of Q . C^T on
// v_mfma_f32_32x32x16_bf16, K in steps of 32 through a two-slot LDS ring.  Candidates are the A operand and queries the B operand, so in the
// C/D layout the query is on the lane (column = lane & 31) and 16 candidates sit in the lane's registers: a lane compares its registers against the ONE
// target score of its query and counts.  A workgroup keeps its 128 queries and walks a slice of the candidate tiles; the counts stay in registers and
// leave once, as integer atomics into the zeroed rank vector (N is cut into slices only to fill the chip; integer adds commute: same result in every run).
//
// The target score t[r] = s[r, labels[r]] comes out of the SAME routine (TARGET = true): its A rows are C[labels[q]] for the workgroup's own queries,
// and the diagonal of the tile is stored.  Every score of a row is therefore the same chain of MFMAs over the same K order, whatever tile it sits
// in: two bit-identical candidate rows get bit-identical scores, and the index rule -- not rounding -- decides between them (metrics.py:156-163).
#include "ocn_common.h"

namespace {

constexpr int RT_CAND = 256;  // candidate rows of a tile (A operand; 2 waves x 4 blocks of 32)
constexpr int RT_QRY = 128;   // query rows of a tile (B operand; 2 waves x 2 blocks of 32)
constexpr int RT_BK = 32;     // K per step
constexpr int RT_LD = 40;     // LDS row stride in elements: 80 bytes = 20 banks, so 16 consecutive rows start on 16 different 4-bank groups (no conflict
                              // among the 16-byte fragment reads of a quarter wave)
constexpr int RT_STAGE = (RT_CAND + RT_QRY) * RT_LD;  // elements of one ring slot (30 KiB)
constexpr int RT_TARGET_WGS = 1024;                   // workgroups the rank launch aims for (two per CU, twice over)

struct RankArgs {
    const bf16* Q;
    const bf16* C;
    const int32_t* labels;  // NULL: labels[r] = r
    float* target;          // TARGET: written; else read
    int32_t* rank;
    int R, N, K;
    int qblocks, ctiles, tiles_per_split;
};

OCN_DEV int rank_label(const RankArgs& a, int q) { return a.labels ? ocn_clamp_index((int)a.labels[q], a.N) : q; }

template <bool TARGET>
__global__ __launch_bounds__(256, 2) void label_rank_kernel(RankArgs a) {
    __shared__ __attribute__((aligned(16))) bf16 smem[2 * RT_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wave >> 1, wq = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int qb = blockIdx.x % a.qblocks, split = blockIdx.x / a.qblocks;
    const int q0 = qb * RT_QRY;
    const int ct_begin = TARGET ? 0 : split * a.tiles_per_split;
    const int ct_end = TARGET ? 1 : min(a.ctiles, ct_begin + a.tiles_per_split);
    const int ksteps = a.K / RT_BK;
    const size_t K = (size_t)a.K;

    // staging: a thread moves 16 bytes of row (tid >> 2) + 64 i, columns 8 (tid & 3) .. + 7: four rows of candidates, two of queries per step
    const int srow = tid >> 2, scol = (tid & 3) * 8;
    const bf16* qptr[2];
    bool qok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = q0 + srow + 64 * i;
        qok[i] = q < a.R;
        qptr[i] = a.Q + (size_t)(qok[i] ? q : 0) * K + scol;
    }
    bf16x8 zero8;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero8[e] = f2bf(0.f);

    // the two queries of this lane (one per 32-block of the wave's 64): their target and label stay in registers for the whole walk
    float tq[2] = {0.f, 0.f};
    int lq[2] = {0, 0}, cnt[2] = {0, 0};
    if (!TARGET) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = q0 + wq * 64 + j * 32 + lr;
            if (q < a.R) {
                tq[j] = a.target[q];
                lq[j] = rank_label(a, q);
            }
        }
    }

    for (int ct = ct_begin; ct < ct_end; ++ct) {
        const int c0 = ct * RT_CAND;
        const bf16* cptr[4];
        bool cok[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = srow + 64 * i;
            int row;
            if (TARGET) {  // row p of the tile is the labelled candidate of query q0 + p; the lower half of the tile stays zero
                cok[i] = p < RT_QRY && q0 + p < a.R;
                row = cok[i] ? rank_label(a, q0 + p) : 0;
            } else {
                cok[i] = c0 + p < a.N;
                row = cok[i] ? c0 + p : 0;
            }
            cptr[i] = a.C + (size_t)row * K + scol;
        }
        f32x16 acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        bf16x8 ra[4], rb[2];
        auto gload = [&](int ks) {  // rows outside the operands are never read: their LDS rows hold zeros
            const int k0 = ks * RT_BK;
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i] = cok[i] ? *(const bf16x8*)(cptr[i] + k0) : zero8;
#pragma unroll
            for (int i = 0; i < 2; ++i) rb[i] = qok[i] ? *(const bf16x8*)(qptr[i] + k0) : zero8;
        };
        auto swrite = [&](int slot) {
            bf16* sA = smem + slot * RT_STAGE;
            bf16* sB = sA + RT_CAND * RT_LD;
#pragma unroll
            for (int i = 0; i < 4; ++i) *(bf16x8*)(sA + (srow + 64 * i) * RT_LD + scol) = ra[i];
#pragma unroll
            for (int i = 0; i < 2; ++i) *(bf16x8*)(sB + (srow + 64 * i) * RT_LD + scol) = rb[i];
        };

        gload(0);
        swrite(0);  // every wave left the previous tile's last slot behind the barrier that ended its K loop
        __syncthreads();
        for (int ks = 0; ks < ksteps; ++ks) {
            const bool more = ks + 1 < ksteps;
            if (more) gload(ks + 1);
            const bf16* sA = smem + (ks & 1) * RT_STAGE;
            const bf16* sB = sA + RT_CAND * RT_LD;
            // TARGET: the lower half of the tile is zero rows whose scores nobody reads -- its two waves skip the fragment reads and MFMAs (a wave-uniform
            // branch) and only stage and meet the barriers; the diagonal's waves run exactly the instructions of the rank launch
            if (!(TARGET && wc == 1))
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16x8 af[4], bq[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *(const bf16x8*)(sA + (wc * 128 + i * 32 + lr) * RT_LD + s * 16 + lh * 8);
#pragma unroll
                for (int j = 0; j < 2; ++j) bq[j] = *(const bf16x8*)(sB + (wq * 64 + j * 32 + lr) * RT_LD + s * 16 + lh * 8);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(af[i], bq[j], acc[i][j]);
            }
            if (more) swrite((ks + 1) & 1);  // the slot that step ks - 1 read: every wave is past the barrier that ended that step
            __syncthreads();
        }

        if (TARGET) {
            // the diagonal: candidate row i * 32 + row meets query wq * 64 + j * 32 + lr at i = 2 wq + j, row = lr -- in the upper half of the tile only
            if (wc == 0) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int q = q0 + wq * 64 + j * 32 + lr;
                    float v = 0.f;
                    bool mine = false;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (i == 2 * wq + j && mfma32_row(r, lane) == lr) {
                                v = acc[i][j][r];
                                mine = true;
                            }
                    if (mine && q < a.R) a.target[q] = v;
                }
            }
        } else {
            // candidate of register r of block i = cb + (i * 32 + (r & 3) + 8 * (r >> 2)): the index tests compare that constant with two per-lane values.
            // Columns past N are never counted (a zero score would beat a negative target): dn is the number of candidates from cb on
            const int cb = c0 + wc * 128 + 4 * lh;
            const int dn = a.N - cb;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int dl = lq[j] - cb;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int k = i * 32 + (r & 3) + 8 * (r >> 2);
                        const float s = acc[i][j][r];
                        const bool beats = (s > tq[j] || (s == tq[j] && k < dl)) && k < dn;
                        cnt[j] += beats ? 1 : 0;
                    }
                    __builtin_amdgcn_sched_barrier(0);  // one block's compare masks at a time: scheduled all at once they spill hundreds of scalar registers
                }
            }
        }
    }

    if (!TARGET) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = q0 + wq * 64 + j * 32 + lr;
            const int v = cnt[j] + __shfl_xor(cnt[j], 32, 64);  // the two lane halves hold different candidates of the same query
            if (lh == 0 && q < a.R && v != 0) atomicAdd(a.rank + q, v);
        }
    }
}

// x fp32 [R, E] -> out bf16 [R, 3 Ep]: hi = bf16(x), lo = bf16(x - hi), zero beyond column E of every segment
__global__ __launch_bounds__(256) void split_bf16x3_kernel(const float* __restrict__ x, bf16* __restrict__ out, long total, int E, int Ep, int role) {
    const long stride = (long)gridDim.x * 256;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const long r = idx / Ep;
        const int e = (int)(idx - r * Ep);
        const float v = e < E ? x[r * E + e] : 0.f;
        const bf16 hi = f2bf(v);
        const bf16 lo = f2bf(v - bf2f(hi));
        bf16* o = out + r * 3 * Ep + e;
        o[0] = hi;
        o[Ep] = role == 0 ? lo : hi;
        o[2 * Ep] = role == 0 ? hi : lo;
    }
}

}  // namespace

extern "C" int ocn_split_bf16x3(const float* x, void* out, int R, int E, int role, ocn_stream_t stream) {
    OCN_CHECK_ARG(x && out, "ocn_split_bf16x3: null operand");
    OCN_CHECK_ARG(R >= 1 && E >= 1, "ocn_split_bf16x3: R=%d and E=%d must be positive", R, E);
    OCN_CHECK_ARG(role == 0 || role == 1, "ocn_split_bf16x3: role=%d must be 0 (query) or 1 (candidate)", role);
    OCN_CHECK_ARG(E <= 0x7fffffff - 31, "ocn_split_bf16x3: E=%d too large", E);
    OCN_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 15) == 0, "ocn_split_bf16x3: x must be 4-byte, out 16-byte aligned");
    const int Ep = (E + 31) / 32 * 32;
    const long total = (long)R * Ep;
    hipLaunchKernelGGL(split_bf16x3_kernel, dim3(ocn_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x, (bf16*)out, total, E, Ep, role);
    OCN_CHECK_LAUNCH("ocn_split_bf16x3");
    return OCN_OK;
}

extern "C" int ocn_label_ranks(const void* Q, const void* C, const int32_t* labels, float* target, int32_t* rank, int R, int N, int K,
                               ocn_stream_t stream) {
    OCN_CHECK_ARG(Q && C && target && rank, "ocn_label_ranks: null operand");
    OCN_CHECK_ARG(R >= 1 && N >= 1, "ocn_label_ranks: R=%d and N=%d must be at least 1", R, N);
    OCN_CHECK_ARG(K >= 32 && K % 32 == 0, "ocn_label_ranks: K=%d must be a multiple of 32", K);
    OCN_CHECK_ARG(N <= 0x7fffffff - 2 * RT_CAND && R <= 0x7fffffff - 2 * RT_QRY, "ocn_label_ranks: R=%d, N=%d too large", R, N);
    OCN_CHECK_ARG(labels || R <= N, "ocn_label_ranks: labels == NULL pairs query r with candidate r, but label %d lies outside [0, N=%d)", R - 1, N);
    OCN_CHECK_ARG(((uintptr_t)Q & 15) == 0 && ((uintptr_t)C & 15) == 0, "ocn_label_ranks: Q and C must be 16-byte aligned");
    OCN_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)target & 3) == 0 && ((uintptr_t)rank & 3) == 0,
                  "ocn_label_ranks: labels, target and rank must be 4-byte aligned");
    RankArgs a;
    a.Q = (const bf16*)Q;
    a.C = (const bf16*)C;
    a.labels = labels;
    a.target = target;
    a.rank = rank;
    a.R = R;
    a.N = N;
    a.K = K;
    a.qblocks = ocn_cdiv(R, RT_QRY);
    a.ctiles = ocn_cdiv(N, RT_CAND);
    int nsplit = ocn_cdiv(RT_TARGET_WGS, a.qblocks);
    nsplit = nsplit < a.ctiles ? nsplit : a.ctiles;
    a.tiles_per_split = ocn_cdiv(a.ctiles, nsplit);
    nsplit = ocn_cdiv(a.ctiles, a.tiles_per_split);
    OCN_CHECK_ARG((long)a.qblocks * nsplit <= 0x7fffffffL, "ocn_label_ranks: R=%d x N=%d too large for one launch", R, N);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(rank, 0, (size_t)R * sizeof(int32_t), st) != hipSuccess) {
        ocn_set_error("ocn_label_ranks: clearing rank failed: %s", hipGetErrorString(hipGetLastError()));
        return OCN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(label_rank_kernel<true>, dim3(a.qblocks), dim3(256), 0, st, a);
    OCN_CHECK_LAUNCH("ocn_label_ranks (targets)");
    hipLaunchKernelGGL(label_rank_kernel<false>, dim3(a.qblocks * nsplit), dim3(256), 0, st, a);
    OCN_CHECK_LAUNCH("ocn_label_ranks");
    return OCN_OK;
}
