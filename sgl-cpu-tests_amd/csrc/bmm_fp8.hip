// bmm_cpu with an fp8 (e4m3fn) mat2 and one per-tensor scale: the per-head products of the MLA absorbed projections
// (q_nope . w_kc, attn_out . w_vc) of fp8 checkpoints, on the matrix pipe.
//
//   out[b][h][n] = bf16( s * sum_k x[b][h][k] * float(w[h][n][k]) )        "heads" = the bmm batch, "rows" = M = B here
//
// fp32 accumulation, the scale applied in fp32 in the epilogue, one rounding to bf16.  w is row-major [H][N][K] or, per
// head, in convert_weight_packed's fp8 order (pack.hip: 1-KiB tiles of 16 rows x 64 k, lane l = row l & 15, k group
// g = l >> 4, bytes 0..7 = k 8g.., bytes 8..15 = k 32 + 8g..).
//
// * arithmetic: fp8 -> bf16 exactly in registers (v_cvt_scalef32_pk_bf16_fp8, scale 1.0), mfma_f32_16x16x32_bf16.  A lane's
//   8 fp8 bytes of one k group are one A operand after conversion, so a packed 16-byte chunk feeds two MFMAs with no shuffle;
//   row-major weights cost two 8-byte loads per lane for the same 64 k.  Both layouts put the same bytes into the same
//   registers in the same order: identical bits.
// * operand roles: weights = A (rows = n), activations = B (columns = m): a lane's four accumulator values are four consecutive
//   n of one row m, stored as one 8-byte bf16 vector, masked per element at the N and M edges.
// * work split: 256 threads = 4 waves, grid (H, ceil(N / 64), ceil(M / (16 MT))).  Wave w owns columns 64 y + 16 w .. + 15 over
//   the whole K for the workgroup's MT in {1, 2, 4} m-subtiles of 16 rows; every converted weight operand is used MT times.
// * weights: global -> registers, never through LDS (no byte is needed by two waves), a ring of kRing 64-k steps in flight
//   per wave that runs ahead across the activation chunks.
// * activations: the workgroup's 16 MT x K block is staged to LDS as bf16, in chunks of kChunk = 1024 / MT columns (33 KiB
//   whatever MT is: four workgroups per CU by LDS), row pitch 2 kChunk + 16 bytes = 4 dwords mod 64 banks, so the 16 lanes of
//   a k group read 16 disjoint 4-bank groups with ds_read_b128.  Rows past M and columns past K hold zeros.
// * K % 8 == 0: a k group of 8 is wholly inside K or wholly zero; 64-k steps past K multiply zeros (K % 64 != 0 exists in the
//   row-major layout only), so the summation order depends on neither the layout nor M.
#include "sglk_common.h"

namespace sglk {
namespace bmm8 {

constexpr int kRing = 4;   // 64-k weight steps in flight per wave

// flags: bit 0 = x may be read in 16-byte vectors, bit 1 = out may be written in 8-byte vectors (pointer and strides aligned)
template <int MT, bool PACKED>
__global__ __launch_bounds__(256) void bmm_heads_fp8_kernel(const uint16_t* __restrict__ x, int64_t x_sb, int64_t x_sh,
                                                            const uint8_t* __restrict__ w, const float* __restrict__ scale,
                                                            uint16_t* __restrict__ out, int64_t o_sb, int64_t o_sh, int M, int N,
                                                            int K, int flags) {
    constexpr int kChunk = 1024 / MT;          // activation columns per LDS chunk
    constexpr int kPitch = 2 * kChunk + 16;    // bytes per LDS row
    constexpr int kSteps = kChunk / 64;        // 64-k steps per chunk: a multiple of kRing, so ring slots stay static
    static_assert(kSteps % kRing == 0, "ring slots must be static across chunks");
    __shared__ __attribute__((aligned(16))) unsigned char xs[16 * MT * kPitch];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int h = blockIdx.x, m0 = blockIdx.z * (16 * MT);
    const int nw = blockIdx.y * 64 + wave * 16;      // first of the wave's 16 output columns
    const bool active = nw < N;                      // a wave wholly past N only helps to stage
    const int nsteps = (K + 63) >> 6;

    // ---- weights: the lane's 16 bytes of 64-k step kp ----
    const uint8_t* wl;                               // packed: the lane's chunk of the wave's first tile; row-major: its row
    const bool row_ok = nw + r < N;
    if (PACKED) wl = w + ((int64_t)h * N + nw) * K + lane * 16;
    else wl = w + ((int64_t)h * N + (row_ok ? nw + r : 0)) * K + 8 * g;
    auto ldw = [&](int kp) __attribute__((always_inline)) -> u32x4 {
        if (PACKED) return *reinterpret_cast<const u32x4*>(wl + (int64_t)kp * 1024);
        const int k = kp * 64 + 8 * g;
        u32x2 lo = {0u, 0u}, hi = {0u, 0u};
        if (row_ok && k < K) lo = *reinterpret_cast<const u32x2*>(wl + kp * 64);
        if (row_ok && k + 32 < K) hi = *reinterpret_cast<const u32x2*>(wl + kp * 64 + 32);
        return (u32x4){lo[0], lo[1], hi[0], hi[1]};
    };
    u32x4 ring[kRing];
#pragma unroll
    for (int i = 0; i < kRing; ++i) ring[i] = (active && i < nsteps) ? ldw(i) : (u32x4){0u, 0u, 0u, 0u};
    const float s = *scale;

    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const uint16_t* xh = x + (int64_t)h * x_sh;
    const unsigned char* xl = xs + r * kPitch + g * 16;   // the lane's B operand of m-subtile 0, k step 0

    for (int kc0 = 0, kpb = 0; kc0 < K; kc0 += kChunk, kpb += kSteps) {
        if (kc0) __syncthreads();                    // every wave is done with the previous chunk
        // ---- stage x[m0 .. m0 + 16 MT)[kc0 .. kc0 + cw * 8) as 16-byte pieces of 8 columns; rows past M, columns past K: zeros ----
        const int kpe = (kpb + kSteps < nsteps) ? kpb + kSteps : nsteps;
        const int cw = (kpe - kpb) * 8;              // pieces per row, whole 64-k steps
        for (int i = tid; i < 16 * MT * cw; i += 256) {
            const int row = i / cw, c = i - row * cw;
            const int m = m0 + row, k = kc0 + c * 8;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m < M && k < K) {
                const uint16_t* src = xh + (int64_t)m * x_sb + k;
                if (flags & 1) {
                    v = *reinterpret_cast<const u32x4*>(src);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = (unsigned)src[2 * q] | ((unsigned)src[2 * q + 1] << 16);
                }
            }
            *reinterpret_cast<u32x4*>(xs + row * kPitch + c * 16) = v;
        }
        __syncthreads();
        if (!active) continue;
        for (int kp0 = kpb; kp0 < kpe; kp0 += kRing) {
#pragma unroll
            for (int i = 0; i < kRing; ++i) {
                const int kp = kp0 + i;
                if (kp < kpe) {
                    const u32x4 cur = ring[i];
                    if (kp + kRing < nsteps) ring[i] = ldw(kp + kRing);
                    const bf16x8 a0 = cvt8(cur[0], cur[1]), a1 = cvt8(cur[2], cur[3]);
                    const unsigned char* xr = xl + (kp - kpb) * 128;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(xr + mt * 16 * kPitch);
                        const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(xr + mt * 16 * kPitch + 64);
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[mt], 0, 0, 0);
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[mt], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (!active) return;

    // ---- epilogue: lane holds out[m0 + 16 mt + r][nw + 4 g .. + 3] ----
    const int n = nw + 4 * g;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m0 + mt * 16 + r;
        if (m >= M || n >= N) continue;
        uint16_t* dst = out + (int64_t)m * o_sb + (int64_t)h * o_sh + n;
        const f32x4 v = acc[mt] * s;
        if ((flags & 2) && n + 3 < N) {
            *reinterpret_cast<u32x2*>(dst) = (u32x2){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (n + i < N) dst[i] = f32_to_bf16_bits(v[i]);
        }
    }
}

template <int MT>
void launch(bool packed, dim3 grid, hipStream_t st, const uint16_t* x, int64_t x_sb, int64_t x_sh, const uint8_t* w,
            const float* scale, uint16_t* out, int64_t o_sb, int64_t o_sh, int M, int N, int K, int flags) {
    if (packed)
        hipLaunchKernelGGL((bmm_heads_fp8_kernel<MT, true>), grid, dim3(256), 0, st, x, x_sb, x_sh, w, scale, out, o_sb, o_sh, M, N,
                           K, flags);
    else
        hipLaunchKernelGGL((bmm_heads_fp8_kernel<MT, false>), grid, dim3(256), 0, st, x, x_sb, x_sh, w, scale, out, o_sb, o_sh, M, N,
                           K, flags);
}

}  // namespace bmm8
}  // namespace sglk

using namespace sglk;

extern "C" int sglk_bmm_heads_fp8(const void* x, int64_t x_stride_b, int64_t x_stride_h, const void* w, int32_t packed,
                                  const float* scale, void* out, int64_t out_stride_b, int64_t out_stride_h, int32_t B, int32_t H,
                                  int32_t OC, int32_t IC, void* stream) {
    SGLK_REQUIRE(B >= 0 && H > 0 && OC > 0 && IC > 0, SGLK_ERR_INVALID, "bmm_heads_fp8: bad sizes B=%d H=%d OC=%d IC=%d", B, H, OC, IC);
    if (B == 0) return SGLK_OK;
    SGLK_REQUIRE(x && w && scale && out, SGLK_ERR_INVALID, "bmm_heads_fp8: null pointer");
    SGLK_REQUIRE(IC % 8 == 0, SGLK_ERR_SHAPE, "bmm_heads_fp8: IC (%d) must be a multiple of 8", IC);
    SGLK_REQUIRE(!packed || (OC % 16 == 0 && IC % 64 == 0), SGLK_ERR_SHAPE,
                 "bmm_heads_fp8: packed weights need OC (%d) %% 16 == 0 and IC (%d) %% 64 == 0", OC, IC);
    SGLK_REQUIRE(((uintptr_t)w % (packed ? 16 : 8)) == 0, SGLK_ERR_INVALID,
                 "bmm_heads_fp8: weights must be %d-byte aligned", packed ? 16 : 8);
    SGLK_REQUIRE(((uintptr_t)x % 2) == 0 && ((uintptr_t)out % 2) == 0 && ((uintptr_t)scale % 4) == 0, SGLK_ERR_INVALID,
                 "bmm_heads_fp8: misaligned x / out / scale");
    const int MT = B <= 16 ? 1 : B <= 32 ? 2 : 4;
    const int64_t gy = ceil_div(OC, 64), gz = ceil_div(B, 16 * MT);
    SGLK_REQUIRE(gy <= 65535 && gz <= 65535, SGLK_ERR_SHAPE, "bmm_heads_fp8: OC (%d) or B (%d) exceeds the launch grid", OC, B);
    const int flags = (((uintptr_t)x % 16) == 0 && x_stride_b % 8 == 0 && x_stride_h % 8 == 0 ? 1 : 0) |
                      (((uintptr_t)out % 8) == 0 && out_stride_b % 4 == 0 && out_stride_h % 4 == 0 ? 2 : 0);
    const dim3 grid((unsigned)H, (unsigned)gy, (unsigned)gz);
    hipStream_t st = (hipStream_t)stream;
#define SGLK_BMM8(MT_)                                                                                                      \
    bmm8::launch<MT_>(packed != 0, grid, st, (const uint16_t*)x, x_stride_b, x_stride_h, (const uint8_t*)w, scale, (uint16_t*)out, \
                      out_stride_b, out_stride_h, B, OC, IC, flags)
    if (MT == 1) SGLK_BMM8(1);
    else if (MT == 2) SGLK_BMM8(2);
    else SGLK_BMM8(4);
#undef SGLK_BMM8
    SGLK_CHECK_LAUNCH("bmm_heads_fp8");
    return SGLK_OK;
}
