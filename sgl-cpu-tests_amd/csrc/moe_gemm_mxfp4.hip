// fused_experts with MX-fp4 (W4A16) expert weights: the two grouped GEMMs on the block-scaled matrix cores with the weights AS
// STORED (E2M1 pairs, element 2i in the low nibble; one E8M0 byte per 32 consecutive elements of a row -- oracle/gemm.py:
// mxfp4_quantize / mxfp4_dequant).  DESIGN.md §10.16.
//
// v_mfma_scale_f32_32x32x64_f8f6f4, operand layout as measured for the dense kernel (gemm_mxfp4.hip): 32 weight rows are the
// fp4 A operand -- lane (r = lane & 31, h = lane >> 5) holds the MX block k = 32h .. 32h+31 of the 64-deep step, 16 contiguous
// bytes of the row, with that block's scale byte in its own scale register -- and 32 slots are the e4m3 B operand.  The
// contract is W4A16: activations go in as two exact e4m3 terms under a power-of-two scale per 128-wide block (fp8_split.h),
// two MFMAs per step, every product exact, fp32 accumulation.  Rounding points: ic1 = silu(gate) * up to bf16, the per-slot
// GEMM-2 row (times its routing weight) to bf16, the combined output (moe_combine.hip).
//
// A workgroup (four waves) owns 128 output columns of one m-tile of the sorted slots (moe_align), in one of two shapes:
//   wide   (128-slot tiles, prefill): wave w = slots [32w, 32w+32) of the tile, all four waves over the SAME weight rows --
//          four 32-row tiles per wave (GATE_UP: four gate + four up = 128 accumulator registers), one k-step of loads ahead;
//   narrow ( 32-slot tiles, decode) : the four waves take DIFFERENT 32-row tiles for the same 32 slots (GATE_UP: one gate + one up
//          tile each), so a handful of slots per expert costs one token tile instead of four mostly empty ones, four times
//          as many workgroups stream weights, and the 32 accumulator registers leave room for a ring of six k-steps
//          (12 KiB of weights per wave) in flight.
// GATE_UP takes gate rows [n0, n0+128) and up rows [N+n0, N+n0+128) of the expert, so silu(g) * u is formed in registers and
// the workgroup holds one WHOLE 128-wide block of ic1 for its slots: the epilogue rounds it to bf16, finds the block maximum
// (inside the wave in the wide shape, through 512 bytes of LDS in the narrow one) and writes the hi / lo e4m3 terms and the
// block's E8M0 byte itself -- GEMM-2 reads operands, no split launch runs over ic1.  Activation rows are gathered through
// sorted_slot / topk from the split copy of `hidden`, which is split once per call (M rows, not M * topk).
// Scales are read one byte per (row tile, k-step) and travel with the step's operands: nothing assumes K % 256 == 0.
// Slots past the tile's rows re-read its last row and are never stored.
#include "fp8_split.h"
#include "knobs.h"
#include "moe_internal.h"

namespace sglk {
namespace mfp4 {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// x [rows][cols] bf16 -> q [rows][hi cols | lo cols] e4m3 in natural k order + one E8M0 byte per 128-wide block.  One wave per
// row, 512 columns per pass: a lane takes 8 columns, 16 lanes one block.  ALIGNED = 16-byte loads (row stride % 8 == 0 and a
// 16-byte aligned base); otherwise element loads, so `hidden` may have any row stride.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void split_rows_kernel(const uint16_t* __restrict__ x, int64_t x_stride, uint8_t* __restrict__ q,
                                                         int64_t q_stride, uint8_t* __restrict__ s, int64_t s_stride, int64_t rows,
                                                         int cols) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint16_t* xr = x + row * x_stride;
    uint8_t* qr = q + row * q_stride;
    for (int c0 = 0; c0 < cols; c0 += 512) {
        const int c = c0 + lane * 8;
        const bool live = c < cols;             // cols % 128 == 0: the 16 lanes of a block are live together
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
        if (live) {
            if constexpr (ALIGNED) {
                const uint4 w4 = *reinterpret_cast<const uint4*>(xr + c);
                const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[2 * i] = __uint_as_float(w[i] << 16);
                    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = bf16_bits_to_f32(xr[c + j]);
            }
        }
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
        const int sb = sp_e8m0_for_amax(amax);
        if (live) {
            if ((lane & 15) == 0) s[row * s_stride + (c >> 7)] = (uint8_t)sb;
            unsigned hi[2], lo[2];
            split8(v, sb, hi, lo);
            *reinterpret_cast<uint2*>(qr + c) = make_uint2(hi[0], hi[1]);
            *reinterpret_cast<uint2*>(qr + cols + c) = make_uint2(lo[0], lo[1]);
        }
    }
}

template <int NT>
struct Step {              // everything one 64-deep k-step of a wave needs
    uint4 a[NT];           // the lane's MX block of each of the wave's row tiles
    unsigned sa[NT];       // ... and its E8M0 byte
    uint4 bh[2], bl[2];    // the slot's activation chunks, hi and lo term
    unsigned sx;           // the slot's E8M0 byte of the 128-wide block the step lies in
};

template <int MODE, bool WIDE>
__global__ __launch_bounds__(256, 2) void moe_gemm_mxfp4_kernel(const Fp4MoeParams p) {
    constexpr int RT = WIDE ? 4 : 1;                              // 32-row tiles per wave (GATE_UP: of gate and of up each)
    constexpr int NT = MODE == MODE_GATE_UP ? 2 * RT : RT;
    constexpr int D = WIDE ? 2 : 6;                               // k-steps in the ring
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;

    const int live = p.num_tiles[0] * p.n_tiles;
    if ((int)blockIdx.x >= live) return;
    const int L = xcd_remap(blockIdx.x, live);
    const int mtile = L / p.n_tiles;
    const int ntile = L - mtile * p.n_tiles;
    const int4 ti = p.tile_info[mtile];
    const int e = __builtin_amdgcn_readfirstlane(ti.x);
    const int pos0 = __builtin_amdgcn_readfirstlane(ti.y);
    const int rows = __builtin_amdgcn_readfirstlane(ti.z);
    const int sg = WIDE ? wave : 0;                               // the wave's group of 32 slots inside the tile
    if (rows <= 0 || (WIDE && sg * 32 >= rows)) return;           // (workgroup-uniform, or the wide shape, which has no barrier)
    const int tr = sg * 32 + r;
    const int trc = tr < rows ? tr : rows - 1;
    const int C = p.C, Ch = C >> 1, Cb = C >> 5;
    const int64_t xrow = MODE == MODE_GATE_UP ? (int64_t)(p.sorted_slot[pos0 + trc] / p.topk) : (int64_t)(pos0 + trc);

    // B operand: bytes 0-15 = k 16h.., bytes 16-31 = k 32+16h.. of the step; 32-bit offsets from the uniform bases (the launch
    // checks that the split rows stay below 4 GiB)
    const unsigned x_off = (unsigned)(xrow * p.x_stride) + 16u * h, xs_off = (unsigned)(xrow * p.xs_stride);
    const uint8_t* xlo_base = p.xq + C;
    const int row0 = ntile * 128 + (WIDE ? 0 : wave * 32);        // first of the wave's output columns
    const uint8_t* wexp = p.w + (int64_t)e * p.w_expert_stride;
    const uint8_t* sexp = p.ws + (int64_t)e * p.ws_expert_stride;
    const unsigned a_off = (unsigned)(r * Ch + 16 * h), s_off = (unsigned)(r * Cb + h);
    // per row tile a wave-uniform base (scalar registers); the lane's part is ONE 32-bit offset shared by all tiles
    const uint8_t* wtile[NT];
    const uint8_t* stile[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int64_t row = (MODE == MODE_GATE_UP && i >= RT) ? p.n_half + row0 + (i - RT) * 32 : row0 + i * 32;
        wtile[i] = wexp + row * Ch;
        stile[i] = sexp + row * Cb;
    }

    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

    auto load_step = [&](int t, Step<NT>& g) __attribute__((always_inline)) {
        const unsigned ao = a_off + 32u * (unsigned)t, so = s_off + 2u * (unsigned)t;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            g.a[i] = *reinterpret_cast<const uint4*>(wtile[i] + ao);
            g.sa[i] = stile[i][so];
        }
        const unsigned xo = x_off + 64u * (unsigned)t;
        g.bh[0] = *reinterpret_cast<const uint4*>(p.xq + xo);
        g.bh[1] = *reinterpret_cast<const uint4*>(p.xq + xo + 32);
        g.bl[0] = *reinterpret_cast<const uint4*>(xlo_base + xo);
        g.bl[1] = *reinterpret_cast<const uint4*>(xlo_base + xo + 32);
        g.sx = p.xs[xs_off + ((unsigned)t >> 1)];
    };
    auto compute = [&](const Step<NT>& g) __attribute__((always_inline)) {
        const i32x8 bh = {(int)g.bh[0].x, (int)g.bh[0].y, (int)g.bh[0].z, (int)g.bh[0].w,
                          (int)g.bh[1].x, (int)g.bh[1].y, (int)g.bh[1].z, (int)g.bh[1].w};
        const i32x8 bl = {(int)g.bl[0].x, (int)g.bl[0].y, (int)g.bl[0].z, (int)g.bl[0].w,
                          (int)g.bl[1].x, (int)g.bl[1].y, (int)g.bl[1].z, (int)g.bl[1].w};
        const int sxh = (int)g.sx, sxl = (int)g.sx - 4;           // the lo term sits four binades down (sx >= 5)
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const i32x8 a = {(int)g.a[i].x, (int)g.a[i].y, (int)g.a[i].z, (int)g.a[i].w, 0, 0, 0, 0};
            acc[i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bh, acc[i], 4, 0, 0, (int)g.sa[i], 0, sxh);
            acc[i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bl, acc[i], 4, 0, 0, (int)g.sa[i], 0, sxl);
        }
    };

    // ring of D k-steps, statically indexed.  The steady loop has no branch between a load and its use; the last D .. 2D-1
    // steps (or all of a reduction shorter than D) drain behind wave-uniform tests.
    const int ns = C >> 6;                                        // >= 2 and even (C % 128 == 0)
    Step<NT> ring[D];
#pragma unroll
    for (int j = 0; j < D; ++j) load_step(j < ns ? j : ns - 1, ring[j]);
    int t0 = 0;
    for (; t0 + 2 * D <= ns; t0 += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            compute(ring[j]);
            load_step(t0 + j + D, ring[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (t0 + j < ns) compute(ring[j]);
        if (t0 + j + D < ns) load_step(t0 + j + D, ring[j]);
    }
#pragma unroll
    for (int j = 0; j < D; ++j)
        if (t0 + D + j < ns) compute(ring[j]);

    // accumulator register i of lane (r, h): output column (i & 3) + 8 (i >> 2) + 4 h of the 32-row tile, slot r of the group
    if constexpr (MODE == MODE_GATE_UP) {
        float v[RT][16];
        float amax = 0.f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float x = bf16_bits_to_f32(f32_to_bf16_bits(silu_f32(acc[rt][i]) * acc[RT + rt][i]));   // ic1's one rounding
                v[rt][i] = x;
                amax = fmaxf(amax, fabsf(x));
            }
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        if constexpr (!WIDE) {                                    // the slot's 128-wide block is spread over the four waves
            __shared__ float xamax[4][32];
            if (h == 0) xamax[wave][r] = amax;
            __syncthreads();
            amax = fmaxf(fmaxf(xamax[0][r], xamax[1][r]), fmaxf(xamax[2][r], xamax[3][r]));
        }
        const int sb = sp_e8m0_for_amax(amax);
        if (tr < rows) {
            const int64_t pos = pos0 + tr;
            if (h == 0 && (WIDE || wave == 0)) p.out_s[pos * p.out_s_stride + ntile] = (uint8_t)sb;
            uint8_t* qhi = p.out_q + pos * p.out_q_stride + row0 + 4 * h;
            uint8_t* qlo = qhi + p.n_half;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {                  // registers 8 gp .. 8 gp + 7: columns 16 gp + 4 h + {0..3, 8..11}
                    unsigned hi[2], lo[2];
                    split8(&v[rt][8 * gp], sb, hi, lo);
                    const int col = rt * 32 + 16 * gp;
                    *reinterpret_cast<unsigned*>(qhi + col) = hi[0];
                    *reinterpret_cast<unsigned*>(qhi + col + 8) = hi[1];
                    *reinterpret_cast<unsigned*>(qlo + col) = lo[0];
                    *reinterpret_cast<unsigned*>(qlo + col + 8) = lo[1];
                }
        }
    } else {
        if (tr >= rows) return;
        const int slot = p.sorted_slot[pos0 + tr];
        const float tw = p.topk_weights[slot];
        uint16_t* orow = p.out + (int64_t)slot * p.out_stride + row0 + 4 * h;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 w;
                w.x = pack_bf16x2(acc[rt][4 * g] * tw, acc[rt][4 * g + 1] * tw);
                w.y = pack_bf16x2(acc[rt][4 * g + 2] * tw, acc[rt][4 * g + 3] * tw);
                *reinterpret_cast<uint2*>(orow + rt * 32 + 8 * g) = w;
            }
    }
}

}  // namespace mfp4

// 128-slot tiles from 8 rows per expert on average.  Measured at E = 128, top-8, N = 768, K = 2048 (tools/probe_moe_mxfp4.py,
// profiles/moe_mxfp4_ops.txt): at 0.25 rows per expert the narrow shape is 12 % faster, at 4 rows the two are level, at 16 rows
// the wide one is 12 % faster although three of its four waves idle in most tiles -- a wide wave feeds eight row tiles from
// one activation fragment, a narrow one two.  SGLK_MXFP4_MOE_TILE = 32 / 128 forces the shape
int mxfp4_moe_tile(int M, int E, int topk) {
    const int f = knobs().mxfp4_moe_tile;
    if (f == 32 || f == 128) return f;
    return (int64_t)M * topk >= (int64_t)8 * E ? 128 : 32;
}

int launch_split_mxfp4_rows(const uint16_t* x, int64_t x_stride, uint8_t* q, int64_t q_stride, uint8_t* s, int64_t s_stride,
                            int64_t rows, int cols, hipStream_t stream) {
    if (rows == 0) return SGLK_OK;
    const dim3 grid((unsigned)ceil_div(rows, 4));
    if (x_stride % 8 == 0 && ((uintptr_t)x % 16) == 0)
        hipLaunchKernelGGL(mfp4::split_rows_kernel<true>, grid, dim3(256), 0, stream, x, x_stride, q, q_stride, s, s_stride, rows, cols);
    else
        hipLaunchKernelGGL(mfp4::split_rows_kernel<false>, grid, dim3(256), 0, stream, x, x_stride, q, q_stride, s, s_stride, rows, cols);
    SGLK_CHECK_LAUNCH("fused_experts(mxfp4): split");
    return SGLK_OK;
}

int launch_moe_gemm_mxfp4(int mode, int tile_m, const Fp4MoeParams& p, int max_mtiles, hipStream_t stream) {
    using namespace mfp4;
    const int64_t blocks = (int64_t)max_mtiles * p.n_tiles;
    if (blocks == 0) return SGLK_OK;
    SGLK_REQUIRE(blocks < (1ll << 31), SGLK_ERR_SHAPE, "fused_experts(mxfp4): too many tiles");
    SGLK_REQUIRE(p.x_rows * p.x_stride < (1ll << 32), SGLK_ERR_SHAPE, "fused_experts(mxfp4): %lld split rows of %lld bytes exceed 4 GiB",
                 (long long)p.x_rows, (long long)p.x_stride);
    SGLK_REQUIRE(p.C % 128 == 0 && (tile_m == 32 || tile_m == 128), SGLK_ERR_SHAPE, "fused_experts(mxfp4): reduction length %d, tile %d", p.C, tile_m);
    const dim3 grid((unsigned)blocks), wg(256);
    if (mode == MODE_GATE_UP) {
        if (tile_m == 128) hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<MODE_GATE_UP, true>), grid, wg, 0, stream, p);
        else hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<MODE_GATE_UP, false>), grid, wg, 0, stream, p);
    } else {
        if (tile_m == 128) hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<MODE_DOWN, true>), grid, wg, 0, stream, p);
        else hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<MODE_DOWN, false>), grid, wg, 0, stream, p);
    }
    SGLK_CHECK_LAUNCH("fused_experts(mxfp4)");
    return SGLK_OK;
}

}  // namespace sglk
