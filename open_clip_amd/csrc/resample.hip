// Antialiased bicubic resampling of uint8 HWC images on the device, one tile routine behind two entry points.
//   ocn_resample_u8: RAGGED sources -- every image of a batch has its own size, lies at its own offset of one byte arena and carries its own
//     description of what to resample: per axis the window of the source the filter may see (top, n), the length R of the virtually resized axis and
//     the slice [o, o + m) of that resized axis that is the output.  The train transform's RandomResizedCrop (window = the box, R = m, o = 0;
//     reference transform.py:435-440) and the validation transform's resize + centre crop / pad (window = the whole image, R from the resize rule,
//     o from the crop; transform.py:461-492) are two uses of that one form.  The plans are made on the host (input_pipeline.eval_resample_plan /
//     train_resample_plan) and travel with the batch; nothing is read back.
//   ocn_resized_crop_u8: sources of ONE size in one tensor and a box per image (input_pipeline.random_resized_crop_boxes): the plan
//     (Hs, Ws, top, left, h, w, Ho, Wo, 0, 0) -- crop first, then resize: the taps are clamped to the box, not to the source.
//
// Per axis: output index o is resized index r = o + oy; r outside [0, R) is the fill colour.  Else scale = n / R, support = 2 max(scale, 1),
// center = scale (r + 0.5), taps k in [max(0, int(center - support + 0.5)), min(n, int(center + support + 0.5))) with weight
// cubic((k - center + 0.5) / max(scale, 1)) (Keys, a = -0.5) divided by their sum; tap k reads source row top + k.
// out = round-half-even(clamp(sum_y sum_x wy wx pixel, 0, 255)), the sum in fp32: F.interpolate(window.float(), mode="bicubic", antialias=True,
// align_corners=False), windowed, clamped and rounded once.  NOT bit-compatible with PIL's fixed-point resampler (which rounds the horizontal pass to
// 8 bits): on noise crops the two differ by at most one level on about a sixth of the values.
//
// One workgroup per (image, tile of 16 output rows x 32 output columns), resample_tile:
//   A  tap ranges (exact integer arithmetic: n (2r + 1) goes up to 2^26, so it stays an int; only the numerator RELATIVE to the first tap, below
//      2^18, becomes a float) and weights of the tile's rows and columns, once, into LDS;
//   B  vertical pass, global uint8 -> fp32 LDS: thread = (output row, 4 consecutive bytes of the source-row span the tile's columns need), the taps
//      in groups of 6 whose loads are in flight together.  How a tap's 4 bytes are loaded is chosen per workgroup, with
//      rows aligned = ((img | row bytes) & 3) == 0 (passes B and C are compiled for either answer, rs_passes<RAGGED, ALIGNED>: a span shift that is
//      a run-time zero on unaligned rows cost the pair path 1 %), and per thread by whether its dword lies in the row:
//                              | rows aligned                       | rows not aligned                      | dword not wholly inside the row
//        crop (RAGGED = false) | one dword per tap, span shifted    | clamped byte loads                    | clamped byte loads
//                              | down by sh = first byte & 3        |                                       |
//        ragged                | one dword per tap with sh, with or | the ALIGNED DWORD PAIR that covers    | clamped byte loads
//                              | without the arena-end clamp        | them, shifted by (address & 3) with   |
//                              |                                    | v_alignbyte_b32, with or without clamp|
//      The crop form reads nothing outside src: its in-row test is the strict q + 4 <= row bytes and it never takes the pair, which can overhang an
//      unaligned src by 3 bytes at either end; the pair is a privilege of the arena, whose base and size are whole dwords.  Bytes a load brings along
//      that no column of the tile needs (in front of the span, behind it, possibly in the next row or the next image) meet weight 0 in pass C;
//   C  horizontal pass out of LDS: thread = 4 consecutive output bytes of one row, stored as one dword where the address allows it.
// boxes, offsets and plan are device data and never checked on the device's behalf by anyone: every size is forced into its range, every source
// coordinate into the image and, in the ragged form, every byte address into the arena (rs_dword / rs_byte) -- see include/openclip_hip.h for the
// resulting semantics.
#include "ocn_common.h"

namespace {

constexpr int RS_TH = 16, RS_TW = 32;  // output tile
constexpr int RS_RATIO = 4;            // largest window side / resized side
constexpr int RS_MAXT = 17;            // taps per axis at that ratio: int(x + 16) - int(x) <= 17
constexpr int RS_GRP = 6;              // taps issued together: their loads are in flight at once (5 or 6 taps per axis at 256 -> 224)
constexpr int RS_WROW = 18;            // floats per weight row: RS_MAXT rounded up to whole groups; the weights behind the last tap are 0
constexpr int RS_IDX = RS_TH + RS_TW;
// floats per row of the intermediate: the tile's columns need at most 4 * (RS_TW - 1) + 17 = 141 source columns = 423 bytes, + 3 of dword alignment
constexpr int RS_SPAN = 432;
constexpr int RS_MAX_OUT = 1024, RS_MAX_SRC = 8192, RS_MAX_R = 4096, RS_PLAN = 10;
constexpr int RS_NEVER = 0x7ffffff0;   // `last` of an image that cannot reach the arena's end (any value above 2^28 is "never")

// what one workgroup resamples: the image (HWC, Hs x Ws), per axis the window (top, nh), the resized length Rh and the output's offset oy in it, every
// entry already inside its range; `last` = the image-relative address of the arena's last dword (RAGGED only)
struct Tile {
    const uint8_t* __restrict__ img;
    int Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox, last;
};

// Keys' cubic convolution kernel, a = -0.5
OCN_DEV float rs_cubic(float x) {
    x = fabsf(x);
    if (x < 1.0f) return (1.5f * x - 2.5f) * x * x + 1.0f;
    if (x < 2.0f) return ((-0.5f * x + 2.5f) * x - 4.0f) * x + 2.0f;
    return 0.0f;
}

// the dword at byte a (a multiple of 4, >= 0) of the image: a dword behind `last` is the arena's last byte four times (= every byte address forced
// to arena_bytes - 1; the arena is whole dwords)
OCN_DEV uint32_t rs_dword(const uint8_t* __restrict__ img, int a, int last) {
    const uint32_t v = *(const uint32_t*)(img + min(a, last));
    return a > last ? (v >> 24) * 0x01010101u : v;
}

// byte q of the source row that starts at image byte `row0` (q may lie outside the row: the column is clamped, the channel kept)
template <bool RAGGED>
OCN_DEV float rs_byte(const uint8_t* __restrict__ img, int row0, int q, int Ws, int last) {
    const int col = (q + 3 * 65536) / 3 - 65536;  // floor(q / 3) for q > -196608 (the corner is held above -32768)
    const int c = q - 3 * col;
    const int a = row0 + ocn_clamp_index(col, Ws) * 3 + c;
    return (float)img[RAGGED ? min(a, last + 3) : a];
}

// the taps of one (output row, 4 source bytes) by dword loads.  PAIR: the 4 bytes straddle two dwords on some row.  CLAMP: the image, or the dword
// behind it, reaches past the arena's end (at most the arena's last image, or a bad offset / plan): only then is an address compared with `last`
template <bool PAIR, bool CLAMP>
OCN_DEV f32x4 rs_column_dwords(const uint8_t* __restrict__ img, int last, int r0, int Hs, int rowbytes, int q, int ny, const float* wrow) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // a whole group of taps at a time, the loads first: a tap behind the last one reads a (clamped, valid) row with weight 0
    for (int k0 = 0; k0 < ny; k0 += RS_GRP) {
        uint32_t v[RS_GRP];
#pragma unroll
        for (int i = 0; i < RS_GRP; ++i) {
            const int a = ocn_clamp_index(r0 + k0 + i, Hs) * rowbytes + q;  // below 2^28: 8192 x 8192 x 3 bytes
            if (PAIR) {
                const uint32_t lo = CLAMP ? rs_dword(img, a & ~3, last) : *(const uint32_t*)(img + (a & ~3));
                const uint32_t hi = CLAMP ? rs_dword(img, (a & ~3) + 4, last) : *(const uint32_t*)(img + (a & ~3) + 4);
                v[i] = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)a & 3u);
            } else {
                v[i] = CLAMP ? rs_dword(img, a, last) : *(const uint32_t*)(img + a);
            }
        }
#pragma unroll
        for (int i = 0; i < RS_GRP; ++i) {
            const float w = wrow[k0 + i];
            const f32x4 p = {(float)(v[i] & 255u), (float)((v[i] >> 8) & 255u), (float)((v[i] >> 16) & 255u), (float)(v[i] >> 24)};
            acc += w * p;
        }
    }
    return acc;
}

// passes B and C of resample_tile, out of the LDS arrays pass A filled.  ALIGNED: every source row starts on a dword, ((img | row bytes) & 3) == 0
template <bool RAGGED, bool ALIGNED>
OCN_DEV void rs_passes(const Tile d, float* __restrict__ inter, const float* __restrict__ wgt, const float* __restrict__ winv, const int* __restrict__ tlo,
                       const int* __restrict__ tn, uint8_t* __restrict__ out, int b, int Ho, int Wo, int fill, int ty, int tx) {
    const int tid = threadIdx.x;
    const uint8_t* __restrict__ img = d.img;
    const int Hs = d.Hs, Ws = d.Ws, top = d.top, left = d.left, Rw = d.Rw, ox = d.ox, last = d.last;
    const int nyo = min(RS_TH, Ho - ty * RS_TH), nxo = min(RS_TW, Wo - tx * RS_TW);
    // the tile's columns that are not fill: [xv0, xv1); their tap ranges move right with the column
    const int xv0 = RAGGED ? min(max(-ox - tx * RS_TW, 0), nxo) : 0, xv1 = RAGGED ? min(max(Rw - ox - tx * RS_TW, 0), nxo) : nxo;
    const bool any = xv0 < xv1;
    const int c_lo = any ? tlo[RS_TH + xv0] : 0, c_hi = any ? tlo[RS_TH + xv1 - 1] + tn[RS_TH + xv1 - 1] : 0;
    const int rowbytes = Ws * 3;
    const int qb0 = (left + c_lo) * 3, qe = (left + c_hi) * 3;  // the span within a source row (outside the row where the window is)
    const int sh = ALIGNED ? (qb0 & 3) : 0;                     // the span starts on a dword; two's complement: also the floor for a negative qb0
    const int qa = qb0 - sh;
    const int ndw = any ? min((max(c_hi - c_lo, 1) * 3 + sh + 3) >> 2, RS_SPAN / 4) : 0;
    // a dword load of pass B starts at most at byte Hs * rowbytes + 3 of the image (the pair's second dword behind the last needed byte of the last row)
    const bool clamp = RAGGED && Hs * rowbytes + 3 > last;

    // ---- B: vertical pass ----
    for (int t = tid; t < nyo * ndw; t += 256) {
        const int y = t / ndw, j = t - y * ndw;
        const int q = qa + 4 * j;
        const int r0 = top + tlo[y], ny = tn[y];
        const float* wrow = wgt + y * RS_WROW;
        // RAGGED: every byte a column needs lies in the row; the others may be anything.  Else: the whole dword lies in the row, hence in src
        const bool dword = RAGGED ? q >= 0 && min(q + 4, qe) <= rowbytes : ALIGNED && q >= 0 && q + 4 <= rowbytes;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (dword) {
            const bool pair = RAGGED && !ALIGNED;
            acc = clamp ? (pair ? rs_column_dwords<true, true>(img, last, r0, Hs, rowbytes, q, ny, wrow)
                                : rs_column_dwords<false, true>(img, last, r0, Hs, rowbytes, q, ny, wrow))
                        : (pair ? rs_column_dwords<true, false>(img, last, r0, Hs, rowbytes, q, ny, wrow)
                                : rs_column_dwords<false, false>(img, last, r0, Hs, rowbytes, q, ny, wrow));
        } else {  // only a window that leaves the source, or a crop out of rows that start on no dword, comes here
            for (int k0 = 0; k0 < ny; k0 += RS_GRP) {
#pragma unroll
                for (int i = 0; i < RS_GRP; ++i) {
                    const int row0 = ocn_clamp_index(r0 + k0 + i, Hs) * rowbytes;
                    const float w = wrow[k0 + i];
                    const f32x4 p = {rs_byte<RAGGED>(img, row0, q, Ws, last), rs_byte<RAGGED>(img, row0, q + 1, Ws, last),
                                     rs_byte<RAGGED>(img, row0, q + 2, Ws, last), rs_byte<RAGGED>(img, row0, q + 3, Ws, last)};
                    acc += w * p;
                }
            }
        }
        *(f32x4*)(inter + y * RS_SPAN + 4 * j) = acc * winv[y];
    }
    __syncthreads();

    // ---- C: horizontal pass ----
    const int nob = nxo * 3, nq = (nob + 3) >> 2;
    const int lim = max(4 * ndw - 1, 0);  // the last float pass B wrote in a row: a tap behind the last one (weight 0) must not meet what LDS held before
    for (int t = tid; t < nyo * nq; t += 256) {
        const int y = t / nq, e0 = 4 * (t - y * nq);
        const bool rowfill = RAGGED && tn[y] < 0;
        uint32_t pk = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = min(e0 + i, nob - 1);
            const int x = e / 3, c = e - 3 * x;
            const bool isfill = RAGGED && (rowfill || tn[RS_TH + x] < 0);
            const int nx = isfill ? 0 : tn[RS_TH + x];
            const int base = (tlo[RS_TH + x] - c_lo) * 3 + c + sh;
            float acc = 0.f;
            for (int k0 = 0; k0 < nx; k0 += RS_GRP) {
#pragma unroll
                for (int j = 0; j < RS_GRP; ++j) acc += wgt[(RS_TH + x) * RS_WROW + k0 + j] * inter[y * RS_SPAN + min(base + 3 * (k0 + j), lim)];
            }
            const float v = __builtin_rintf(__builtin_amdgcn_fmed3f(acc * winv[RS_TH + x], 0.f, 255.f));  // round to nearest, ties to even
            pk |= (isfill ? (uint32_t)fill : (uint32_t)v) << (8 * i);
        }
        uint8_t* o = out + ((size_t)(b * (size_t)Ho + ty * RS_TH + y) * Wo + tx * RS_TW) * 3 + e0;
        if (e0 + 4 <= nob && ((uintptr_t)o & 3) == 0) {
            *(uint32_t*)o = pk;
        } else {
            for (int i = 0; i < 4 && e0 + i < nob; ++i) o[i] = (uint8_t)(pk >> (8 * i));
        }
    }
}

// one 16 x 32 tile (ty, tx) of output image b: pass A here, then B and C.  RAGGED = false: no fill (oy = ox = 0 and R = the output's side), no arena end
template <bool RAGGED>
OCN_DEV void resample_tile(const Tile d, uint8_t* __restrict__ out, int b, int Ho, int Wo, int fill, int ty, int tx) {
    __shared__ __attribute__((aligned(16))) float inter[RS_TH * RS_SPAN];
    __shared__ float wgt[RS_IDX * RS_WROW], winv[RS_IDX];
    __shared__ int tlo[RS_IDX], tn[RS_IDX], tnum[RS_IDX];  // tn: the tap count; -1: a fill row / column; 0: behind the output's edge
    const int tid = threadIdx.x;
    const int nh = d.nh, nw = d.nw, Rh = d.Rh, Rw = d.Rw, oy = d.oy, ox = d.ox;

    // ---- A: taps of the tile's rows (idx < RS_TH) and columns.  With M = max(n, R): center - support + 0.5 = (n (2r + 1) - 4M + R) / 2R and the argument
    // of tap lo + k is ((2 (lo + k) + 1) R - n (2r + 1)) / 2M -- integer numerators, one fp32 division each ----
    if (tid < RS_IDX) {
        const bool isy = tid < RS_TH;
        const int o = isy ? ty * RS_TH + tid : tx * RS_TW + (tid - RS_TH);
        const int r = o + (isy ? oy : ox);
        const int n = isy ? nh : nw, m = isy ? Rh : Rw, M = max(n, m);
        const bool inside = o < (isy ? Ho : Wo), valid = inside && (!RAGGED || (r >= 0 && r < m));
        const int c2 = n * (2 * (valid ? r : 0) + 1);
        const int lo = max(0, (c2 - 4 * M + m) / (2 * m));  // a negative numerator truncates towards 0: at most 0 either way
        const int hi = min(n, (c2 + 4 * M + m) / (2 * m));
        tlo[tid] = lo;
        tn[tid] = valid ? max(min(hi - lo, RS_MAXT), 0) : (inside ? -1 : 0);
        tnum[tid] = (2 * lo + 1) * m - c2;
    }
    __syncthreads();
    const float deny = (float)(2 * max(nh, Rh)), denx = (float)(2 * max(nw, Rw));
    for (int t = tid; t < RS_IDX * RS_WROW; t += 256) {
        const int idx = t / RS_WROW, k = t - idx * RS_WROW;
        const bool isy = idx < RS_TH;
        const int num = tnum[idx] + 2 * k * (isy ? Rh : Rw);
        wgt[t] = k < tn[idx] ? rs_cubic((float)num / (isy ? deny : denx)) : 0.f;
    }
    __syncthreads();
    if (tid < RS_IDX) {  // the weights stay as they are; each pass multiplies its sum by 1 / (sum of the weights)
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < RS_WROW; ++k) s += wgt[tid * RS_WROW + k];
        winv[tid] = s != 0.f ? 1.0f / s : 0.f;
    }
    __syncthreads();

    if ((((uintptr_t)d.img | (uintptr_t)(d.Ws * 3)) & 3) == 0) rs_passes<RAGGED, true>(d, inter, wgt, winv, tlo, tn, out, b, Ho, Wo, fill, ty, tx);
    else rs_passes<RAGGED, false>(d, inter, wgt, winv, tlo, tn, out, b, Ho, Wo, fill, ty, tx);
}

__global__ __launch_bounds__(256) void resized_crop_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ boxes,
                                                              uint8_t* __restrict__ out, int Hs, int Ws, int Ho, int Wo, int nty, int ntx) {
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = bid % ntx, ty = (bid / ntx) % nty, b = bid / (ntx * nty);
    // the box: sides into [1, 4 m]; the corner into a range in which top + row cannot overflow (beyond +-32768 every row clamps to the same edge)
    const int32_t* __restrict__ bx = boxes + 4 * (size_t)b;
    const Tile d = {src + (size_t)b * Hs * Ws * 3, Hs, Ws, min(max(bx[0], -32768), 32768), min(max(bx[1], -32768), 32768),
                    min(max(bx[2], 1), RS_RATIO * Ho), min(max(bx[3], 1), RS_RATIO * Wo), Ho, Wo, 0, 0, RS_NEVER};
    resample_tile<false>(d, out, b, Ho, Wo, 0, ty, tx);
}

__global__ __launch_bounds__(256) void resample_u8_kernel(const uint8_t* __restrict__ arena, long long arena_bytes, const long long* __restrict__ offsets,
                                                          const int32_t* __restrict__ plan, uint8_t* __restrict__ out, int Ho, int Wo, int fill,
                                                          int nty, int ntx) {
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = bid % ntx, ty = (bid / ntx) % nty, b = bid / (ntx * nty);
    // the plan, every entry into its range: sizes into [1, 8192], resized sides into [1, 4096], window sides into [1, min(4 R, 8192)], the corner and the
    // output offset into ranges in which no sum can overflow (beyond them every row clamps to the same edge / every pixel is fill anyway)
    const int32_t* __restrict__ pl = plan + (size_t)b * RS_PLAN;
    const int Rh = min(max(pl[6], 1), RS_MAX_R), Rw = min(max(pl[7], 1), RS_MAX_R);
    // the image: its offset into [0, arena_bytes - 4], down to a dword; `last` = the arena's last dword relative to it
    const long long base = min(max(offsets[b], 0LL), arena_bytes - 4) & ~3LL;
    const Tile d = {arena + base, min(max(pl[0], 1), RS_MAX_SRC), min(max(pl[1], 1), RS_MAX_SRC), min(max(pl[2], -32768), 32768),
                    min(max(pl[3], -32768), 32768), min(max(pl[4], 1), min(RS_RATIO * Rh, RS_MAX_SRC)), min(max(pl[5], 1), min(RS_RATIO * Rw, RS_MAX_SRC)),
                    Rh, Rw, min(max(pl[8], -RS_MAX_R), RS_MAX_R), min(max(pl[9], -RS_MAX_R), RS_MAX_R),
                    (int)min(arena_bytes - 4 - base, (long long)RS_NEVER)};
    resample_tile<true>(d, out, b, Ho, Wo, fill, ty, tx);
}

}  // namespace

extern "C" int ocn_resized_crop_u8(const void* src_u8, int B, int Hs, int Ws, const int32_t* boxes, void* out_u8, int Ho, int Wo,
                                   ocn_stream_t stream) {
    OCN_CHECK_ARG(src_u8 && boxes && out_u8, "ocn_resized_crop_u8: null operand");
    OCN_CHECK_ARG(((uintptr_t)boxes & 3) == 0, "ocn_resized_crop_u8: boxes must be 4-byte aligned");
    OCN_CHECK_ARG(B > 0 && Ho >= 1 && Ho <= RS_MAX_OUT && Wo >= 1 && Wo <= RS_MAX_OUT,
                  "ocn_resized_crop_u8: bad output shape B=%d Ho=%d Wo=%d (B >= 1, 1 <= Ho, Wo <= %d)", B, Ho, Wo, RS_MAX_OUT);
    OCN_CHECK_ARG(Hs >= 1 && Hs <= RS_MAX_SRC && Ws >= 1 && Ws <= RS_MAX_SRC, "ocn_resized_crop_u8: bad source shape Hs=%d Ws=%d (1 <= Hs, Ws <= %d)",
                  Hs, Ws, RS_MAX_SRC);
    const int nty = ocn_cdiv(Ho, RS_TH), ntx = ocn_cdiv(Wo, RS_TW);
    const long nwg = (long)B * nty * ntx;
    OCN_CHECK_ARG(nwg <= 0x7fffffffL, "ocn_resized_crop_u8: B=%d images of %d x %d tiles exceed the grid", B, nty, ntx);
    hipLaunchKernelGGL(resized_crop_u8_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src_u8, boxes, (uint8_t*)out_u8,
                       Hs, Ws, Ho, Wo, nty, ntx);
    OCN_CHECK_LAUNCH("ocn_resized_crop_u8");
    return OCN_OK;
}

extern "C" int ocn_resample_u8(const void* arena_u8, int64_t arena_bytes, const int64_t* offsets, const int32_t* plan, int B, void* out_u8, int Ho, int Wo,
                               int fill, ocn_stream_t stream) {
    OCN_CHECK_ARG(arena_u8 && offsets && plan && out_u8, "ocn_resample_u8: null operand");
    OCN_CHECK_ARG(((uintptr_t)arena_u8 & 15) == 0, "ocn_resample_u8: the arena must be 16-byte aligned");
    OCN_CHECK_ARG(arena_bytes >= 4 && (arena_bytes & 3) == 0, "ocn_resample_u8: arena_bytes=%lld must be a positive multiple of 4", (long long)arena_bytes);
    OCN_CHECK_ARG(((uintptr_t)offsets & 7) == 0, "ocn_resample_u8: offsets must be 8-byte aligned");
    OCN_CHECK_ARG(((uintptr_t)plan & 3) == 0, "ocn_resample_u8: plan must be 4-byte aligned");
    OCN_CHECK_ARG(B > 0 && Ho >= 1 && Ho <= RS_MAX_OUT && Wo >= 1 && Wo <= RS_MAX_OUT,
                  "ocn_resample_u8: bad output shape B=%d Ho=%d Wo=%d (B >= 1, 1 <= Ho, Wo <= %d)", B, Ho, Wo, RS_MAX_OUT);
    OCN_CHECK_ARG(fill >= 0 && fill <= 255, "ocn_resample_u8: fill=%d must lie in [0, 255]", fill);
    const int nty = ocn_cdiv(Ho, RS_TH), ntx = ocn_cdiv(Wo, RS_TW);
    const long nwg = (long)B * nty * ntx;
    OCN_CHECK_ARG(nwg <= 0x7fffffffL, "ocn_resample_u8: B=%d images of %d x %d tiles exceed the grid", B, nty, ntx);
    hipLaunchKernelGGL(resample_u8_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)arena_u8, (long long)arena_bytes,
                       (const long long*)offsets, plan, (uint8_t*)out_u8, Ho, Wo, fill, nty, ntx);
    OCN_CHECK_LAUNCH("ocn_resample_u8");
    return OCN_OK;
}
