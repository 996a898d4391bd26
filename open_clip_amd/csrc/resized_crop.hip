// RandomResizedCrop on the device (reference transform.py:435-440: RandomResizedCrop(image_size, scale, interpolation=BICUBIC) of the train
// transform): crop a box out of every decoded uint8 source image and resize it to the model's size with the ANTIALIASED bicubic filter, rounded
// once.  The boxes are drawn on the host (input_pipeline.random_resized_crop_boxes) and travel with the batch; nothing is read back.
//
// Per axis (box side n, output side m): scale = n / m, support = 2 max(scale, 1), inv = 1 / max(scale, 1); output index o has
// center = scale (o + 0.5), taps k in [max(0, int(center - support + 0.5)), min(n, int(center + support + 0.5))) with weight
// cubic((k - center + 0.5) inv) (Keys, a = -0.5) divided by their sum.  Taps are clamped to the CROP (crop first, then resize).
// out = round-half-even(clamp(sum_y sum_x wy wx pixel, 0, 255)), the sum in fp32: F.interpolate(crop.float(), mode="bicubic", antialias=True,
// align_corners=False) + clamp + round.  NOT bit-compatible with PIL's fixed-point resampler (which rounds the horizontal pass to 8 bits):
// on noise the two differ by at most one level on about a sixth of the values.
//
// One workgroup per (image, tile of 16 output rows x 32 output columns):
//   A  tap ranges (exact integer arithmetic) and weights of the tile's 16 rows and 32 columns, once, into LDS;
//   B  vertical pass, global uint8 -> fp32 LDS: thread = (output row, 4 consecutive bytes of the source-row span the tile's columns need);
//      one aligned dword load per tap where the source rows are dword-aligned, four clamped byte loads elsewhere;
//   C  horizontal pass out of LDS: thread = 4 consecutive output bytes of one row, stored as one dword where the address allows it.
// Box contents are device data: a side is forced into [1, 4 m] (at most 17 taps per axis; anchored at the top-left corner) and every source
// coordinate into the image, so no lane reads outside src whatever boxes holds (a box that reaches outside sees the edge pixel repeated).
#include "ocn_common.h"

namespace {

constexpr int RC_TH = 16, RC_TW = 32;  // output tile
constexpr int RC_RATIO = 4;            // largest box side / output side
constexpr int RC_MAXT = 17;            // taps per axis at that ratio: int(x + 16) - int(x) <= 17
constexpr int RC_GRP = 6;              // taps issued together: their loads are in flight at once (5 or 6 taps per axis at 256 -> 224)
constexpr int RC_WROW = 18;            // floats per weight row: RC_MAXT rounded up to whole groups; the weights behind the last tap are 0
constexpr int RC_IDX = RC_TH + RC_TW;
// floats per row of the intermediate: the tile's columns need at most 4 * (RC_TW - 1) + 17 = 141 source columns = 423 bytes, + 3 of dword alignment
constexpr int RC_SPAN = 432;
constexpr int RC_MAX_OUT = 1024, RC_MAX_SRC = 8192;

// Keys' cubic convolution kernel, a = -0.5
OCN_DEV float rc_cubic(float x) {
    x = fabsf(x);
    if (x < 1.0f) return (1.5f * x - 2.5f) * x * x + 1.0f;
    if (x < 2.0f) return ((-0.5f * x + 2.5f) * x - 4.0f) * x + 2.0f;
    return 0.0f;
}

// byte q of a source row (q may lie outside the row: the column is clamped, the channel kept)
OCN_DEV float rc_byte(const uint8_t* __restrict__ row, int q, int Ws) {
    const int col = (q + 3 * 65536) / 3 - 65536;  // floor(q / 3) for q > -196608 (the corner is held above -32768)
    const int c = q - 3 * col;
    return (float)row[ocn_clamp_index(col, Ws) * 3 + c];
}

__global__ __launch_bounds__(256) void resized_crop_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ boxes,
                                                              uint8_t* __restrict__ out, int Hs, int Ws, int Ho, int Wo, int nty, int ntx) {
    __shared__ __attribute__((aligned(16))) float inter[RC_TH * RC_SPAN];
    __shared__ float wgt[RC_IDX * RC_WROW], winv[RC_IDX];
    __shared__ int tlo[RC_IDX], tn[RC_IDX], tnum[RC_IDX];
    const int tid = threadIdx.x;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = bid % ntx, ty = (bid / ntx) % nty, b = bid / (ntx * nty);
    // the box: sides into [1, 4 m]; the corner into a range in which top + row cannot overflow (beyond +-32768 every row clamps to the same edge)
    const int top = min(max(boxes[4 * b + 0], -32768), 32768), left = min(max(boxes[4 * b + 1], -32768), 32768);
    const int bh = min(max(boxes[4 * b + 2], 1), RC_RATIO * Ho), bw = min(max(boxes[4 * b + 3], 1), RC_RATIO * Wo);

    // ---- A: taps of the tile's rows (idx < RC_TH) and columns.  With M = max(n, m): center - support + 0.5 = (n (2o + 1) - 4M + m) / 2m and the argument
    // of tap lo + k is ((2 (lo + k) + 1) m - n (2o + 1)) / 2M -- integer numerators (below 2^24), one fp32 division each ----
    if (tid < RC_IDX) {
        const bool isy = tid < RC_TH;
        const int o = isy ? ty * RC_TH + tid : tx * RC_TW + (tid - RC_TH);
        const int n = isy ? bh : bw, m = isy ? Ho : Wo, M = max(n, m);
        const int c2 = n * (2 * o + 1);
        const int lo = max(0, (c2 - 4 * M + m) / (2 * m));  // a negative numerator truncates towards 0: at most 0 either way
        const int hi = min(n, (c2 + 4 * M + m) / (2 * m));
        tlo[tid] = lo;
        tn[tid] = o < m ? max(min(hi - lo, RC_MAXT), 0) : 0;
        tnum[tid] = (2 * lo + 1) * m - c2;
    }
    __syncthreads();
    const float deny = (float)(2 * max(bh, Ho)), denx = (float)(2 * max(bw, Wo));
    for (int t = tid; t < RC_IDX * RC_WROW; t += 256) {
        const int idx = t / RC_WROW, k = t - idx * RC_WROW;
        const bool isy = idx < RC_TH;
        const int num = tnum[idx] + 2 * k * (isy ? Ho : Wo);
        wgt[t] = k < tn[idx] ? rc_cubic((float)num / (isy ? deny : denx)) : 0.f;
    }
    __syncthreads();
    if (tid < RC_IDX) {  // the weights stay as they are; each pass multiplies its sum by 1 / (sum of the weights)
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < RC_WROW; ++k) s += wgt[tid * RC_WROW + k];
        winv[tid] = s != 0.f ? 1.0f / s : 0.f;
    }
    __syncthreads();

    const int nyo = min(RC_TH, Ho - ty * RC_TH), nxo = min(RC_TW, Wo - tx * RC_TW);
    const int c_lo = tlo[RC_TH], c_hi = tlo[RC_TH + nxo - 1] + tn[RC_TH + nxo - 1];  // the tap ranges move right with the column
    const int rowbytes = Ws * 3;
    const bool aligned = (((uintptr_t)src | (uintptr_t)rowbytes) & 3) == 0;  // every source row starts on a dword
    const int qb0 = (left + c_lo) * 3;             // first byte of the span within a source row (outside the row when the box is)
    const int sh = aligned ? (qb0 & 3) : 0;        // two's complement: also the floor for a negative qb0
    const int qa = qb0 - sh;
    const int ndw = min((max(c_hi - c_lo, 1) * 3 + sh + 3) >> 2, RC_SPAN / 4);
    const uint8_t* __restrict__ img = src + (size_t)b * Hs * rowbytes;

    // ---- B: vertical pass ----
    for (int t = tid; t < nyo * ndw; t += 256) {
        const int y = t / ndw, j = t - y * ndw;
        const int q = qa + 4 * j;
        const int r0 = top + tlo[y], ny = tn[y];
        const bool dword = aligned && q >= 0 && q + 4 <= rowbytes;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        // a whole group of taps at a time, the loads first: a tap behind the last one reads a (clamped, valid) row with weight 0
        for (int k0 = 0; k0 < ny; k0 += RC_GRP) {
            if (dword) {
                uint32_t v[RC_GRP];
#pragma unroll
                for (int i = 0; i < RC_GRP; ++i) v[i] = *(const uint32_t*)(img + (size_t)ocn_clamp_index(r0 + k0 + i, Hs) * rowbytes + q);
#pragma unroll
                for (int i = 0; i < RC_GRP; ++i) {
                    const float w = wgt[y * RC_WROW + k0 + i];
                    const f32x4 p = {(float)(v[i] & 255u), (float)((v[i] >> 8) & 255u), (float)((v[i] >> 16) & 255u), (float)(v[i] >> 24)};
                    acc += w * p;
                }
            } else {
#pragma unroll
                for (int i = 0; i < RC_GRP; ++i) {
                    const uint8_t* __restrict__ row = img + (size_t)ocn_clamp_index(r0 + k0 + i, Hs) * rowbytes;
                    const float w = wgt[y * RC_WROW + k0 + i];
                    const f32x4 p = {rc_byte(row, q, Ws), rc_byte(row, q + 1, Ws), rc_byte(row, q + 2, Ws), rc_byte(row, q + 3, Ws)};
                    acc += w * p;
                }
            }
        }
        *(f32x4*)(inter + y * RC_SPAN + 4 * j) = acc * winv[y];
    }
    __syncthreads();

    // ---- C: horizontal pass ----
    const int nob = nxo * 3, nq = (nob + 3) >> 2;
    const int lim = 4 * ndw - 1;  // the last float pass B wrote in a row: a tap behind the last one (weight 0) must not meet what LDS held before
    for (int t = tid; t < nyo * nq; t += 256) {
        const int y = t / nq, e0 = 4 * (t - y * nq);
        uint32_t pk = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = min(e0 + i, nob - 1);
            const int x = e / 3, c = e - 3 * x;
            const int nx = tn[RC_TH + x];
            const int base = (tlo[RC_TH + x] - c_lo) * 3 + c + sh;
            float acc = 0.f;
            for (int k0 = 0; k0 < nx; k0 += RC_GRP) {
#pragma unroll
                for (int j = 0; j < RC_GRP; ++j) acc += wgt[(RC_TH + x) * RC_WROW + k0 + j] * inter[y * RC_SPAN + min(base + 3 * (k0 + j), lim)];
            }
            const float v = __builtin_rintf(__builtin_amdgcn_fmed3f(acc * winv[RC_TH + x], 0.f, 255.f));  // round to nearest, ties to even
            pk |= (uint32_t)v << (8 * i);
        }
        uint8_t* o = out + ((size_t)(b * (size_t)Ho + ty * RC_TH + y) * Wo + tx * RC_TW) * 3 + e0;
        if (e0 + 4 <= nob && ((uintptr_t)o & 3) == 0) {
            *(uint32_t*)o = pk;
        } else {
            for (int i = 0; i < 4 && e0 + i < nob; ++i) o[i] = (uint8_t)(pk >> (8 * i));
        }
    }
}

}  // namespace

extern "C" int ocn_resized_crop_u8(const void* src_u8, int B, int Hs, int Ws, const int32_t* boxes, void* out_u8, int Ho, int Wo,
                                   ocn_stream_t stream) {
    OCN_CHECK_ARG(src_u8 && boxes && out_u8, "ocn_resized_crop_u8: null operand");
    OCN_CHECK_ARG(((uintptr_t)boxes & 3) == 0, "ocn_resized_crop_u8: boxes must be 4-byte aligned");
    OCN_CHECK_ARG(B > 0 && Ho >= 1 && Ho <= RC_MAX_OUT && Wo >= 1 && Wo <= RC_MAX_OUT,
                  "ocn_resized_crop_u8: bad output shape B=%d Ho=%d Wo=%d (B >= 1, 1 <= Ho, Wo <= %d)", B, Ho, Wo, RC_MAX_OUT);
    OCN_CHECK_ARG(Hs >= 1 && Hs <= RC_MAX_SRC && Ws >= 1 && Ws <= RC_MAX_SRC, "ocn_resized_crop_u8: bad source shape Hs=%d Ws=%d (1 <= Hs, Ws <= %d)",
                  Hs, Ws, RC_MAX_SRC);
    const int nty = ocn_cdiv(Ho, RC_TH), ntx = ocn_cdiv(Wo, RC_TW);
    const long nwg = (long)B * nty * ntx;
    OCN_CHECK_ARG(nwg <= 0x7fffffffL, "ocn_resized_crop_u8: B=%d images of %d x %d tiles exceed the grid", B, nty, ntx);
    hipLaunchKernelGGL(resized_crop_u8_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src_u8, boxes, (uint8_t*)out_u8,
                       Hs, Ws, Ho, Wo, nty, ntx);
    OCN_CHECK_LAUNCH("ocn_resized_crop_u8");
    return OCN_OK;
}
