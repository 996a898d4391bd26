// Muon optimizer (open_clip_amd/optim.py::NativeMuon): the batched small-tile NT GEMM of the Newton-Schulz iteration and the three HBM-bound
// multi-tensor kernels around it (momentum + norm, normalise into the bf16 workspace, apply + operand-copy refresh).
//
// Per 2-D weight [rows, cols] (a 4-D weight as [shape[0], -1]) and step, in fp32 unless marked:
//   g = grad * clip;  buf += (1 - momentum) (g - buf);  u = nesterov ? g + momentum (buf - g) : buf;  X = bf16(u / (||u||_F + 1e-7))
//   ns_steps times:  A = X X^T;  B = b A + c A A;  X = a X + B X      (bf16 operands, fp32 accumulation, ONE rounding per stored matrix)
//   w = w (1 - lr wd) - lr scale X
// X lives in the workspace as its [rows, cols] image ("natural", row stride pad32(cols)) AND its transposed image (row stride pad32(rows)):
// the iteration runs on whichever of the two is wide ([min, max]), and its last product needs the other one as the [N, K] operand of the NT form.
// Both are zero-padded to multiples of 32; zero rows and columns are invariant under the iteration, so the padding is exact.
// No fp32 atomic anywhere: ||u||^2 is one partial per 64x64 tile, folded per matrix by one workgroup in a fixed order.
#include "ocn_common.h"

namespace {

// ---- C_i[M,N] = bf16(alpha A_i[M,K] B_i[N,K]^T + beta R_i[M,N]), optionally also C_i^T ---------------------------------------------------
// One workgroup (4 waves, 2 x 2) per 128 x 128 tile of one problem; K in steps of 32 through a two-slot LDS ring (the structure of
// retrieval.hip's tile routine).  The MFMA takes the B rows as its first operand, so in the C/D layout the lane owns ONE row m of C
// (lane & 31) and every register quad four consecutive columns n: the stores of C and the loads of R are 8-byte vectors, the transposed
// store runs along m across the lanes.
constexpr int GB_T = 128;   // tile edge
constexpr int GB_BK = 32;   // K per step
constexpr int GB_LD = 40;   // LDS row stride in elements (80 bytes: conflict-free 16-byte fragment reads, see retrieval.hip)
constexpr int GB_STAGE = 2 * GB_T * GB_LD;  // elements of one ring slot (20 KiB)

struct GemmBatchedArgs {
    const bf16* A; const bf16* B; bf16* C; const bf16* R; bf16* Ct;
    long sA, sB, sC, sR, sCt;
    int lda, ldb, ldc, ldr, ldct;
    int M, N, K, tiles_m, tiles_n;
    float alpha, beta;
};

__global__ __launch_bounds__(256, 2) void gemm_nt_batched_kernel(GemmBatchedArgs a) {
    __shared__ __attribute__((aligned(16))) bf16 smem[2 * GB_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int tiles = a.tiles_m * a.tiles_n;
    const int prob = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int m0 = (t / a.tiles_n) * GB_T, n0 = (t % a.tiles_n) * GB_T;
    const bf16* A = a.A + (size_t)prob * a.sA;
    const bf16* B = a.B + (size_t)prob * a.sB;
    const int ksteps = a.K / GB_BK;

    // staging: a thread moves 16 bytes of row (tid >> 2) + 64 i, columns 8 (tid & 3) .. + 7 of both operands; rows outside are never read
    const int srow = tid >> 2, scol = (tid & 3) * 8;
    const bf16* aptr[2];
    const bf16* bptr[2];
    bool aok[2], bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + srow + 64 * i, n = n0 + srow + 64 * i;
        aok[i] = m < a.M;
        bok[i] = n < a.N;
        aptr[i] = A + (size_t)(aok[i] ? m : 0) * a.lda + scol;
        bptr[i] = B + (size_t)(bok[i] ? n : 0) * a.ldb + scol;
    }
    bf16x8 zero8;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero8[e] = f2bf(0.f);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    bf16x8 ra[2], rb[2];
    auto gload = [&](int ks) {
        const int k0 = ks * GB_BK;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ra[i] = aok[i] ? *(const bf16x8*)(aptr[i] + k0) : zero8;
            rb[i] = bok[i] ? *(const bf16x8*)(bptr[i] + k0) : zero8;
        }
    };
    auto swrite = [&](int slot) {
        bf16* sA = smem + slot * GB_STAGE;
        bf16* sB = sA + GB_T * GB_LD;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *(bf16x8*)(sA + (srow + 64 * i) * GB_LD + scol) = ra[i];
            *(bf16x8*)(sB + (srow + 64 * i) * GB_LD + scol) = rb[i];
        }
    };

    gload(0);
    swrite(0);
    __syncthreads();
    for (int ks = 0; ks < ksteps; ++ks) {
        const bool more = ks + 1 < ksteps;
        if (more) gload(ks + 1);
        const bf16* sA = smem + (ks & 1) * GB_STAGE;
        const bf16* sB = sA + GB_T * GB_LD;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 af[2], bq[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = *(const bf16x8*)(sA + (wm * 64 + i * 32 + lr) * GB_LD + s * 16 + lh * 8);
#pragma unroll
            for (int j = 0; j < 2; ++j) bq[j] = *(const bf16x8*)(sB + (wn * 64 + j * 32 + lr) * GB_LD + s * 16 + lh * 8);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(bq[j], af[i], acc[i][j]);  // register rows = n, lane column = m
        }
        if (more) swrite((ks + 1) & 1);  // the slot that step ks - 1 read: every wave is past the barrier that ended that step
        __syncthreads();
    }

    bf16* C = a.C + (size_t)prob * a.sC;
    const bf16* R = a.R ? a.R + (size_t)prob * a.sR : nullptr;
    bf16* Ct = a.Ct ? a.Ct + (size_t)prob * a.sCt : nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 64 + i * 32 + lr;
        if (m >= a.M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 64 + j * 32 + 8 * q + 4 * lh;  // columns n .. n + 3: registers 4 q .. 4 q + 3
                if (n >= a.N) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = a.alpha * acc[i][j][4 * q + e];
                if (n + 3 < a.N) {
                    if (R) {
                        const bf16x4 r4 = *(const bf16x4*)(R + (size_t)m * a.ldr + n);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaf(a.beta, bf2f(r4[e]), v[e]);
                    }
                    *(bf16x4*)(C + (size_t)m * a.ldc + n) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                    if (Ct)
#pragma unroll
                        for (int e = 0; e < 4; ++e) Ct[(size_t)(n + e) * a.ldct + m] = f2bf(v[e]);
                } else {
                    for (int e = 0; e < 4 && n + e < a.N; ++e) {
                        const float x = R ? fmaf(a.beta, bf2f(R[(size_t)m * a.ldr + n + e]), v[e]) : v[e];
                        C[(size_t)m * a.ldc + n + e] = f2bf(x);
                        if (Ct) Ct[(size_t)(n + e) * a.ldct + m] = f2bf(x);
                    }
                }
            }
    }
}

// ---- multi-tensor kernels: one workgroup per 64 x 64 tile of a weight's [rows, cols] view (ragged edges guarded) ---------------------------
struct MuonEntry {
    const float* g;
    float* buf;
    float* w;
    bf16* w16n;      // cached operand copy [rows, cols] or NULL
    bf16* w16t;      // cached transposed copy [cols, rows] or NULL (only for 64-multiple shapes)
    bf16* xn;        // workspace: natural image of X, [pad32(rows)] x ldn -- written by normalize
    bf16* xt;        // workspace: transposed image, [pad32(cols)] x ldt -- written by normalize
    const bf16* xfin;  // natural image of the LAST iterate -- read by apply
    int rows, cols, ldn, ldt;
    int chunk0, nchunks;  // this matrix's slots of the partial-sum workspace
    float step, decay;    // lr * scale;  1 - lr * weight_decay
};
static_assert(sizeof(MuonEntry) == 96, "MuonEntry layout is mirrored by open_clip_amd/optim.py");

// the update direction from the clipped gradient and the UPDATED buffer (one definition: momentum and normalize must agree to the bit)
OCN_DEV float muon_u(float g, float buf, float momentum, int nesterov) { return nesterov ? __fmaf_rn(momentum, buf - g, g) : buf; }

struct TilePos {
    int r0, c0, tx, ty;
};
OCN_DEV TilePos tile_pos(const MuonEntry& e, int idx) {
    const int tiles_c = (e.cols + 63) >> 6;
    return {(idx / tiles_c) * 64, (idx % tiles_c) * 64, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6)};
}

__global__ __launch_bounds__(256) void muon_momentum_kernel(const MuonEntry* __restrict__ entries, const int2* __restrict__ chunks, float momentum,
                                                            int nesterov, const float* __restrict__ gnorm_sq, float max_norm,
                                                            float* __restrict__ chunk_ws) {
    __shared__ float red[4];
    const int2 ch = chunks[blockIdx.x];
    const MuonEntry e = entries[ch.x];
    const TilePos p = tile_pos(e, ch.y);
    const float gs = grad_clip_coef(gnorm_sq, max_norm);
    float s = 0.f;
    const int c = p.c0 + p.tx;
    if (c < e.cols)
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int r = p.r0 + p.ty + 4 * i;
            if (r < e.rows) {
                const size_t o = (size_t)r * e.cols + c;
                const float g = e.g[o] * gs;
                float b = e.buf[o];
                b = b + (g - b) * (1.0f - momentum);
                e.buf[o] = b;
                const float u = muon_u(g, b, momentum, nesterov);
                s = __fmaf_rn(u, u, s);
            }
        }
    const float t = block_sum_256(s, red);
    if (threadIdx.x == 0) chunk_ws[e.chunk0 + ch.y] = t;
}

// inv_norm[i] = 1 / (sqrt(sum of matrix i's partials) + 1e-7): one workgroup per matrix, the additions in one fixed order (as sumsq_fold_kernel)
__global__ __launch_bounds__(256) void muon_fold_kernel(const MuonEntry* __restrict__ entries, const float* __restrict__ chunk_ws,
                                                        float* __restrict__ inv_norm) {
    __shared__ float red[4];
    const MuonEntry e = entries[blockIdx.x];
    float s = 0.f;
    for (int i = threadIdx.x; i < e.nchunks; i += 256) s += chunk_ws[e.chunk0 + i];
    const float t = block_sum_256(s, red);
    if (threadIdx.x == 0) inv_norm[blockIdx.x] = 1.0f / (sqrtf(t) + 1e-7f);
}

// X = bf16(u * inv_norm) into both workspace images; everything of the tile inside the padded images and outside the matrix is written as zero
__global__ __launch_bounds__(256) void muon_normalize_kernel(const MuonEntry* __restrict__ entries, const int2* __restrict__ chunks, float momentum,
                                                             int nesterov, const float* __restrict__ gnorm_sq, float max_norm,
                                                             const float* __restrict__ inv_norm) {
    __shared__ bf16 tile[64][66];
    const int2 ch = chunks[blockIdx.x];
    const MuonEntry e = entries[ch.x];
    const TilePos p = tile_pos(e, ch.y);
    const float gs = grad_clip_coef(gnorm_sq, max_norm), inv = inv_norm[ch.x];
    const int rp = (e.rows + 31) & ~31, cp = (e.cols + 31) & ~31;  // padded extents: rp <= ldt, cp <= ldn
    const int c = p.c0 + p.tx;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int rl = p.ty + 4 * i, r = p.r0 + rl;
        float x = 0.f;
        if (r < e.rows && c < e.cols) {
            const size_t o = (size_t)r * e.cols + c;
            x = muon_u(e.g[o] * gs, e.buf[o], momentum, nesterov) * inv;
        }
        const bf16 xb = f2bf(x);
        tile[rl][p.tx] = xb;
        if (r < rp && c < cp) e.xn[(size_t)r * e.ldn + c] = xb;
    }
    __syncthreads();
    const int r = p.r0 + p.tx;  // the transposed image: lanes run along the rows of the weight
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int cl = p.ty + 4 * i, cc = p.c0 + cl;
        if (cc < cp && r < rp) e.xt[(size_t)cc * e.ldt + r] = tile[p.tx][cl];
    }
}

// w = w * decay - step * X, plus the bf16 operand copies ([rows, cols] and, through LDS, [cols, rows]) in the same pass
__global__ __launch_bounds__(256) void muon_apply_kernel(const MuonEntry* __restrict__ entries, const int2* __restrict__ chunks) {
    __shared__ bf16 tile[64][66];
    const int2 ch = chunks[blockIdx.x];
    const MuonEntry e = entries[ch.x];
    const TilePos p = tile_pos(e, ch.y);
    const int c = p.c0 + p.tx;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int rl = p.ty + 4 * i, r = p.r0 + rl;
        if (r < e.rows && c < e.cols) {
            const size_t o = (size_t)r * e.cols + c;
            const float x = bf2f(e.xfin[(size_t)r * e.ldn + c]);
            const float w = e.w[o] * e.decay - e.step * x;
            e.w[o] = w;
            const bf16 wb = f2bf(w);
            if (e.w16n) e.w16n[o] = wb;
            tile[rl][p.tx] = wb;
        }
    }
    if (e.w16t) {  // rows, cols % 64 == 0 (the host passes the transposed copy only then): the tile is full
        __syncthreads();
        const int r = p.r0 + p.tx;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int cl = p.ty + 4 * i;
            e.w16t[(size_t)(p.c0 + cl) * e.rows + r] = tile[p.tx][cl];
        }
    }
}

// out = bf16(acc + beta * R) (and its transpose): the second half of a Newton-Schulz statement when the product came from ocn_gemm_nt (per-matrix backend)
__global__ __launch_bounds__(256) void muon_axpby_kernel(const float* __restrict__ acc, const bf16* __restrict__ R, bf16* __restrict__ out,
                                                         bf16* __restrict__ outT, int rows, int cols, float beta) {
    const long total = (long)rows * cols, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const bf16 v = f2bf(fmaf(beta, bf2f(R[i]), acc[i]));
        out[i] = v;
        if (outT) {
            const long r = i / cols;
            outT[(i - r * cols) * rows + r] = v;
        }
    }
}

}  // namespace

extern "C" int ocn_gemm_nt_batched(const void* A, int lda, int64_t strideA, const void* B, int ldb, int64_t strideB, void* C, int ldc, int64_t strideC,
                                   const void* R, int ldr, int64_t strideR, void* Ct, int ldct, int64_t strideCt, int M, int N, int K, int batch,
                                   float alpha, float beta, ocn_stream_t stream) {
    OCN_CHECK_ARG(A && B && C, "ocn_gemm_nt_batched: null operand");
    OCN_CHECK_ARG(M >= 1 && N >= 1 && batch >= 1, "ocn_gemm_nt_batched: M=%d, N=%d and batch=%d must be positive", M, N, batch);
    OCN_CHECK_ARG(K >= 32 && K % 32 == 0, "ocn_gemm_nt_batched: K=%d must be a multiple of 32", K);
    OCN_CHECK_ARG(lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && (!R || ldr % 8 == 0), "ocn_gemm_nt_batched: row strides must be multiples of 8");
    OCN_CHECK_ARG(lda >= K && ldb >= K && ldc >= N && (!R || ldr >= N) && (!Ct || ldct >= M), "ocn_gemm_nt_batched: a row stride is shorter than its row");
    OCN_CHECK_ARG(strideA % 8 == 0 && strideB % 8 == 0 && strideC % 8 == 0 && strideR % 8 == 0 && strideA >= 0 && strideB >= 0 && strideC >= 0 &&
                      strideR >= 0 && strideCt >= 0,
                  "ocn_gemm_nt_batched: batch strides must be non-negative multiples of 8");
    OCN_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0 && ((uintptr_t)C & 15) == 0 && ((uintptr_t)R & 15) == 0 && ((uintptr_t)Ct & 1) == 0,
                  "ocn_gemm_nt_batched: A, B, C and R must be 16-byte aligned");
    GemmBatchedArgs a;
    a.A = (const bf16*)A; a.B = (const bf16*)B; a.C = (bf16*)C; a.R = (const bf16*)R; a.Ct = (bf16*)Ct;
    a.sA = strideA; a.sB = strideB; a.sC = strideC; a.sR = strideR; a.sCt = strideCt;
    a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldr = ldr; a.ldct = ldct;
    a.M = M; a.N = N; a.K = K;
    a.tiles_m = ocn_cdiv(M, GB_T);
    a.tiles_n = ocn_cdiv(N, GB_T);
    a.alpha = alpha; a.beta = beta;
    const long grid = (long)batch * a.tiles_m * a.tiles_n;
    OCN_CHECK_ARG(grid <= 0x7fffffffL, "ocn_gemm_nt_batched: batch=%d x M=%d x N=%d too large for one launch", batch, M, N);
    hipLaunchKernelGGL(gemm_nt_batched_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    OCN_CHECK_LAUNCH("ocn_gemm_nt_batched");
    return OCN_OK;
}

extern "C" int ocn_muon_momentum_multi(const void* entries, int n_entries, const void* chunks, int n_chunks, float momentum, int nesterov,
                                       const float* gnorm_sq, float max_norm, float* chunk_ws, float* inv_norm, ocn_stream_t stream) {
    OCN_CHECK_ARG(entries && chunks && chunk_ws && inv_norm && n_entries > 0 && n_chunks > 0, "ocn_muon_momentum_multi: bad arguments");
    hipLaunchKernelGGL(muon_momentum_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const MuonEntry*)entries, (const int2*)chunks,
                       momentum, nesterov, gnorm_sq, max_norm, chunk_ws);
    OCN_CHECK_LAUNCH("ocn_muon_momentum_multi");
    hipLaunchKernelGGL(muon_fold_kernel, dim3(n_entries), dim3(256), 0, (hipStream_t)stream, (const MuonEntry*)entries, chunk_ws, inv_norm);
    OCN_CHECK_LAUNCH("ocn_muon_momentum_multi (fold)");
    return OCN_OK;
}

extern "C" int ocn_muon_normalize_multi(const void* entries, const void* chunks, int n_chunks, float momentum, int nesterov, const float* gnorm_sq,
                                        float max_norm, const float* inv_norm, ocn_stream_t stream) {
    OCN_CHECK_ARG(entries && chunks && inv_norm && n_chunks > 0, "ocn_muon_normalize_multi: bad arguments");
    hipLaunchKernelGGL(muon_normalize_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const MuonEntry*)entries, (const int2*)chunks,
                       momentum, nesterov, gnorm_sq, max_norm, inv_norm);
    OCN_CHECK_LAUNCH("ocn_muon_normalize_multi");
    return OCN_OK;
}

extern "C" int ocn_muon_apply_multi(const void* entries, const void* chunks, int n_chunks, ocn_stream_t stream) {
    OCN_CHECK_ARG(entries && chunks && n_chunks > 0, "ocn_muon_apply_multi: bad arguments");
    hipLaunchKernelGGL(muon_apply_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const MuonEntry*)entries, (const int2*)chunks);
    OCN_CHECK_LAUNCH("ocn_muon_apply_multi");
    return OCN_OK;
}

extern "C" int ocn_muon_axpby(const float* acc, const void* R, void* out, void* outT, int rows, int cols, float beta, ocn_stream_t stream) {
    OCN_CHECK_ARG(acc && R && out && rows > 0 && cols > 0, "ocn_muon_axpby: bad arguments");
    hipLaunchKernelGGL(muon_axpby_kernel, dim3(ocn_grid_for((long)rows * cols, 256)), dim3(256), 0, (hipStream_t)stream, acc, (const bf16*)R,
                       (bf16*)out, (bf16*)outT, rows, cols, beta);
    OCN_CHECK_LAUNCH("ocn_muon_axpby");
    return OCN_OK;
}
