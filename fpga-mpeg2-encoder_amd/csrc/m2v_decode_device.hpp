// m2v_decode_device.hpp — the device code the decode units share, once: where a chunk's picture lies (slot), the sink a slice walk
// stores dec::IMb records through and its twin that stores nothing, the reconstruction of one dec::IMb macroblock, and the loop that
// packs one picture into a byte range of the caller's buffer.  Everything here is a __device__ function that its kernels inline: a
// kernel is launched from the unit that holds it, finds its record, weights and slots, and calls one of these.
// The module-syntax kernels (dec::MbRec with `mode`: k_dec_recon, k_dm_recon, k_ds_recon) and k_db_recon (dec::BMb, dec::bp_predict)
// predict differently and keep their bodies; k_dec_out and k_ds_out walk several frames per 16-byte unit and keep theirs.
#pragma once
#include "m2v_decode_kernels.hpp"

namespace m2v {

constexpr uint32_t kNoPic = 0xFFFFFFFFu;

// the chunk's slot of the picture (or frame) with index r: the chunk's own from slot 2 on, the last anchor in front of the chunk (c1)
// in slot 1, the one before it in slot 0
__device__ inline uint32_t slot(uint32_t r, uint32_t p0, uint32_t c1) { return r == kNoPic ? 0u : r >= p0 ? 2u + (r - p0) : r == c1 ? 1u : 0u; }

// what a slice walk leaves per macroblock: the record, six DC values, the quantised levels as dense int16 [6][64], raster order
struct IMbSink {
    dec::IMb *mb_;
    int32_t *dc_;
    int16_t *lv_;
    M2V_HD void mb(int col, const dec::IMb &m, const int32_t (&dc)[6])
    {
        mb_[col] = m;
#pragma unroll
        for (int k = 0; k < 6; ++k) dc_[col * 6 + k] = dc[k];
    }
    M2V_HD void level(int col, int blk, uint32_t i, int32_t l) { lv_[(col * 6 + blk) * 64 + (int)i] = (int16_t)l; }
};
struct IMbNoSink {                                 // a walk for the verdict alone
    M2V_HD void mb(int, const dec::IMb &, const int32_t (&)[6]) {}
    M2V_HD void level(int, int, uint32_t, int32_t) {}
};

// one wavefront, lane l: macroblock m's coded blocks into F - a lane per coefficient dequantises (weights: the intra matrix, then the
// non-intra one, raster order; mismatch control through one ballot), 48 lanes run the rows and then the columns.  Ends behind a barrier
__device__ inline void imb_residual(int32_t (&F)[6][64], const dec::IMb m, const dec::PicParams pp, const uint8_t *__restrict__ weights,
                                    const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, size_t at, uint32_t l)
{
    const bool intra = m.intra != 0;
    const int32_t qscale = dec::main_scale(m.qcode, pp.qst), weight = weights[(intra ? 0u : 64u) + l];
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) {
        if (!((m.cbp >> (5 - blk)) & 1)) continue;                     // (uniform: the whole wavefront works on one macroblock)
        int32_t f = intra && l == 0 ? dec::main_dequant_dc(dc[at * 6 + blk], pp.prec) : dec::main_dequant(lv[(at * 6 + blk) * 64 + l], weight, intra, qscale);
        const int odd = __popcll(__ballot(f & 1)) & 1;
        if (!odd && l == 63) f = dec::mismatch(f);
        F[blk][l] = f;
    }
    __syncthreads();
    const int blk8 = (int)(l >> 3), r8 = (int)(l & 7u);
    const bool mine = l < 48 && ((m.cbp >> (5 - blk8)) & 1);
    if (mine) {
        int32_t a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = F[blk8][r8 * 8 + j];
        dec::idct_1d(a, true, dec::kIso);
#pragma unroll
        for (int j = 0; j < 8; ++j) F[blk8][r8 * 8 + j] = a[j];
    }
    __syncthreads();
    if (mine) {
        int32_t a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = F[blk8][j * 8 + r8];
        dec::idct_1d(a, false, dec::kIso);
#pragma unroll
        for (int j = 0; j < 8; ++j) F[blk8][j * 8 + r8] = a[j];
    }
    __syncthreads();
}

// one wavefront per macroblock of a frame picture: record mb[at] at (col, row) of the picture at cur, W x H samples of whole
// macroblocks with chroma lines of CW; its predictions read the pictures at fwd and bwd (dec::il_predict)
__device__ inline void imb_recon(int32_t (&F)[6][64], const dec::IMb m, const dec::PicParams pp, const uint8_t *__restrict__ weights,
                                 const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, size_t at, uint8_t *cur, const uint8_t *fwd, const uint8_t *bwd,
                                 uint32_t W, uint32_t H, uint32_t CW, uint32_t col, uint32_t row, uint32_t l)
{
    imb_residual(F, m, pp, weights, dc, lv, at, l);
    const bool intra = m.intra != 0;
    {   // luma: four samples of one row per lane; the row's block and the row inside it through the field-DCT map
        const uint32_t y = l >> 2, x0 = (l & 3u) * 4u, blk = dec::il_luma_block(x0, y, m.dct_type), brow = dec::il_luma_row(y, m.dct_type);
        const bool coded = (m.cbp >> (5 - blk)) & 1;
        const int px = (int)(16u * col + x0), py = (int)(16u * row + y);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t pred = intra ? 128 : dec::il_predict(fwd, bwd, (int)W, px + j, py, m, false);
            const int32_t res = coded ? F[blk][brow * 8u + ((x0 + j) & 7u)] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint32_t *)(cur + (size_t)(16u * row + y) * W + 16u * col + x0) = v;
    }
    {   // chroma: two samples per lane, U in the first half of the wavefront; frame blocks always
        const uint32_t pl = l >> 5, y = (l >> 2) & 7u, x0 = (l & 3u) * 2u;
        const bool coded = (m.cbp >> (1 - pl)) & 1;
        const size_t plane = (size_t)W * H + (size_t)pl * CW * (H / 2u);
        const int px = (int)(8u * col + x0), py = (int)(8u * row + y);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int32_t pred = intra ? 128 : dec::il_predict(fwd + plane, bwd + plane, (int)CW, px + j, py, m, true);
            const int32_t res = coded ? F[4u + pl][y * 8u + x0 + j] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint16_t *)(cur + plane + (size_t)(8u * row + y) * CW + 8u * col + x0) = (uint16_t)v;
    }
}

typedef uint32_t store_t __attribute__((ext_vector_type(4)));

// the picture at pic (W x H samples of whole macroblocks, w x h of them shown) into bytes [lo, hi) of dst, over a grid of blocks of
// `threads` lanes.  A 16-byte unit of the destination that lies inside the range is one aligned store; the units at its edges go byte
// by byte, so two frames that share a unit never write each other's bytes
__device__ inline void out_picture(const uint8_t *__restrict__ pic, uint32_t w, uint32_t h, uint32_t W, uint32_t H, unsigned long long lo, unsigned long long hi,
                                   uint8_t *__restrict__ dst, int layout, uint32_t threads)
{
    const unsigned long long lead = (unsigned long long)(uintptr_t)dst & 15ull;
    const unsigned long long u0 = (lo + lead) >> 4, u1 = (hi + lead + 15ull) >> 4;
    for (unsigned long long g = u0 + (unsigned long long)blockIdx.x * threads + threadIdx.x; g < u1; g += (unsigned long long)gridDim.x * threads) {
        const long long o0 = (long long)(g << 4) - (long long)lead;
        const int k0 = o0 < (long long)lo ? (int)((long long)lo - o0) : 0, k1 = (long long)hi - o0 < 16 ? (int)((long long)hi - o0) : 16;
        if (k0 >= k1) continue;
        uint32_t q = (uint32_t)((unsigned long long)(o0 + k0) - lo);
        dec::OutAt at = dec::out_locate(q, w, h, layout);
        uint32_t v[4] = {0, 0, 0, 0};
        for (int k = k0; k < k1; ++k) {
            v[k >> 2] |= (uint32_t)dec::pic_sample(pic, W, H, at) << (8 * (k & 3));
            if (k + 1 == k1) break;
            ++q;
            if (at.run > 1) dec::out_step(at, layout);
            else at = dec::out_locate(q, w, h, layout);
        }
        if (k0 == 0 && k1 == 16) {
            *(__attribute__((address_space(1))) store_t *)(dst + o0) = store_t{v[0], v[1], v[2], v[3]};
        } else {
            for (int k = k0; k < k1; ++k) dst[o0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        }
    }
}

}  // namespace m2v
