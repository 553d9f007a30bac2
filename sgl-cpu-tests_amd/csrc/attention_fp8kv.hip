// decode_attention_fp8kv: one-token paged attention over a float8_e4m3fn KV cache with one scale per tensor.
//
//   1. k_buffer[loc[b]] = e4m3(clamp(float(key[b]) / k_scale, +-448)), v_buffer likewise (quantising write kernel below)
//   2. out[b, h] = v_scale * softmax_j(cap(sm_scale * k_scale * q[b, h] . float(K[j]))) @ float(V[j])
//
// The cache bytes are never expanded in memory: they travel HBM -> LDS as bytes and become bf16 (exactly) in registers, right
// in front of mfma_f32_16x16x32_bf16.  k_scale rides in the softmax scale, v_scale in each split's 1 / l, so the partials, the
// log-sum-exps and decode_merge_kernel (attention.hip) are those of the bf16 operator.
//
// * image: a tile is 64 keys x D bytes, row-major, D / 16 chunks of 16 bytes per row (36, 8, 12, 4); MLA: 36 KiB (the
//   value columns are its first 512 bytes per row), GQA 128: 8 + 8 KiB.  Rows arrive by LDS-DMA, 16 bytes per lane, linear
//   image, swizzle applied to the SOURCE chunk; the page ids of a tile by a DMA of their own two steps ahead of its rows
//   (ring of 8 tables).  kBufs = 3 tiles ring (112.6 KiB for MLA): at the wait for tile t the rows of t+1 and t+2 are in
//   flight (the bf16 kernel holds two tiles in 144 KiB).  Counted s_waitcnt vmcnt(n) and bare s_barrier as there; 2304 chunks
//   over 512 threads is 4.5 rounds, so waves 0-3 issue five instructions per tile, waves 4-7 four, and the counts follow.
// * swizzle (byte elements): both LDS reads below fetch one chunk column of 16 rows per 256 bytes = all 64 banks: Q.K rows
//   16 kt .. + 15 (ds_read_b128: a 16-lane service group), P.V rows {32 ss + 16 a + 4 g + b} of two lane groups g (one
//   ds_read_b64_tr_b8 pass of 32 lanes) = rows 0-7 and 16-23, or 8-15 and 24-31, of a 32-key half.  With v(r) = r[2:0] |
//   (r[3] ^ r[4]) << 3 both sets carry 16 distinct v.  A row starts at chunk slot (D / 16) r mod 16 of the 16 slots that
//   span the banks:  D / 16 = 4, 12, 36: 4 (+-r mod 4) -> XOR the chunk with v[3:2] (stays inside an aligned group of 4);
//   D / 16 = 8: 8 (r & 1) -> XOR with v[3:1];  D / 16 = 32 (an unaliased 512-wide V): 0 -> XOR with v[3:0].
// * Q.K^T: K is the A operand.  Lane (key r = l & 15, g = l >> 4) reads chunk 4 s + g of its row with ONE ds_read_b128: bytes
//   0-7 convert to the A operand of MFMA 2s, bytes 8-15 to that of MFMA 2s + 1, no shuffle; q is loaded once in the same
//   order (MFMA 2s + h, lane group g: q[64 s + 16 g + 8 h .. + 7]).
// * P.V: ds_read_b64_tr_b8 (mapping: tools/probe/ds_read_tr8_probe.hip, profiles/ds_read_tr8_probe.txt -- inside 16 lanes, lane i
//   supplies 8 bytes of row i >> 1, half i & 1 of an 8 x 16 byte block and receives column i).  Lane group g supplies the
//   keys its P registers hold (4 g .. + 3 of two 16-key tiles), so one read + one cvt8 is the A operand of 16 value columns x
//   32 keys.  Inline asm with hand-counted lgkmcnt, three reads ahead (the builtin makes the compiler drain vmcnt, i.e.
//   the tiles in flight).  P is rounded to bf16, sums and accumulators are fp32, as in attention.hip's core.
// * work split, priced per 64-key MLA tile (22 heads: 2 column tiles; a CU has ~3600 cycles per 36 KiB at 24.6 GB/s,
//   a 16x16x32 MFMA is 16 cycles of a SIMD's matrix pipe, a cvt8 4 VALU instructions = 16 cycles of its VALU):
//     8 waves = 2 key halves x 2 column tiles x 2 value slices (the bf16 split): per wave 36 + 16 MFMAs and as many cvt8
//       -> 832 matrix + 832 VALU cycles (+ ~150 softmax) if a conversion instruction issued at full rate, two waves per SIMD
//       -> ~1700-2000 cycles when the two overlap.  Measured: 3.3 us (~7900 cycles) per tile, what the 416 conversions per SIMD
//       cost at QUARTER rate (supposed, not counted) -- more slices would only add conversions;
//     2 key halves x 2 column tiles x ONE slice on 4 waves: 36 + 32 per wave, one wave per SIMD -> 1088 + 1088 cycles with
//       nothing to overlap them, and a 128-register accumulator beside 72 registers of q;
//     4 key quarters: P.V's k-step is 32 keys, a 16-key wave would multiply half zeros.
//   Kept: 2 x 2 x 2 for wide heads (logits computed twice, 288 of 416 MFMAs per tile).  Narrow heads (D <= 192) recomputed
//   the logits in each of FOUR value slices; with a conversion on every K byte that is the larger part, so they now run as
//   2 key halves x 2 slices on 4 waves (D = 128, 16 heads: 12 MFMAs + 12 cvt8 per wave and tile instead of 20 + 20).
//   Wide heads with more than 32 q heads per kv head take two workgroups per kv head (32 heads each).
#include "attention_internal.h"
#include "knobs.h"

namespace sglk {
namespace attn8 {

typedef const __attribute__((address_space(1))) void* dma_gptr_t;
typedef __attribute__((address_space(3))) void* dma_lptr_t;
typedef __attribute__((address_space(3))) unsigned char* lds_u8_ptr;

constexpr int kKeys = 64;     // keys per tile
constexpr int kIdRing = 8;    // page-id tables (64 ids each)
constexpr int kLdsMax = 160 * 1024;

// XOR mask of row r's 16-byte chunks for an image of CH chunks per row (file header)
template <int CH>
SGLK_DEV int swz(int r) {
    const int v = (r & 7) | ((((r >> 3) ^ (r >> 4)) & 1) << 3);
    if constexpr (CH % 16 == 0) return v;
    else if constexpr (CH % 16 == 8) return v >> 1;
    else { static_assert(CH % 4 == 0, "chunks per row must be a multiple of 4"); return v >> 2; }
}

template <int N> SGLK_DEV void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// LDS-DMA of one 64-row tile of WIDTH bytes per row by THREADS threads: FULL rounds of every wave and, when the chunk count
// leaves half a round, one more by the first XW waves.  Rows past the tile's keys repeat its last row (the id table does).
template <int WIDTH, int THREADS>
struct RowDma {
    static constexpr int CH = WIDTH / 16;
    static constexpr int FULL = kKeys * CH / THREADS;
    static constexpr int XW = (kKeys * CH - FULL * THREADS) / 64;
    static_assert(kKeys * CH == FULL * THREADS + XW * 64, "whole wave instructions only");
    template <int AUX>   // 2 = non-temporal
    SGLK_DEV static void issue(unsigned char* lds, const unsigned char* buf, int64_t stride_tok, const unsigned* ids, int wave, int lane) {
        constexpr int N = FULL + (XW ? 1 : 0);
        int tok[N];
#pragma unroll
        for (int i = 0; i < N; ++i) tok[i] = (int)ids[((i * THREADS + wave * 64 + lane) / CH) & (kKeys - 1)];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i == FULL && wave >= XW) break;
            const int c = i * THREADS + wave * 64 + lane;
            const int row = c / CH, slot = c - row * CH;
            const unsigned char* g = buf + (int64_t)tok[i] * stride_tok + ((slot ^ swz<CH>(row)) << 4);
            __builtin_amdgcn_global_load_lds((dma_gptr_t)g, (dma_lptr_t)(lds + (i * THREADS + wave * 64) * 16), 16, 0, AUX);
        }
    }
};

struct Params {
    const unsigned short* q;
    const unsigned char *k_buf, *v_buf;
    int64_t q_s0, q_s1, kb_s0, kb_s1, vb_s0, vb_s1;   // q in elements, caches in bytes
    float* logits;          // [B][HQ][logit_splits][DV+1]
    const void* req_to_token;
    int64_t rtt_stride;
    int rtt_is64;
    const int64_t* b_req_idx;
    const int64_t* b_seq_len;
    int HQ, HKV, splits, logit_splits;
    float scale_log2e;      // sm_scale * k_scale * log2(e)
    float logit_cap, v_scale;
    int nt;                 // cache rows are read non-temporal (SGLK_DEC_NT)
    unsigned short* o;      // direct: one split -> the kernel rounds and stores the output itself
    int64_t o_s0, o_s1;
    int direct;
};

// Per-wave state: 16 q heads (columns) x NKT 16-key tiles of every 64-key tile x DVW value columns.
template <int D, int DVW, int NKT>
struct Core8 {
    static constexpr int KS = D / 64;       // 64-wide k steps of Q.K (two MFMAs each)
    static constexpr int VT = DVW / 16;
    bf16x8 qf[KS][2];
    f32x4 o[VT];
    float m, l;

    SGLK_DEV void init() {
        m = -INFINITY;
        l = 0.f;
#pragma unroll
        for (int t = 0; t < VT; ++t) o[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    SGLK_DEV void load_q(const unsigned short* qrow, int lane) {   // nullptr = padding column
        const int g = lane >> 4;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (qrow) v = *reinterpret_cast<const uint4*>(qrow + ks * 64 + g * 16 + h * 8);
                qf[ks][h] = __builtin_bit_cast(bf16x8, v);
            }
    }

    // keys k0 .. k0 + 16 NKT of the tile at klds; V columns from chunk vc0 of the image at vlds (VCH chunks per row);
    // `limit`: the lane's column sees stream positions < limit
    template <int VCH>
    SGLK_DEV void tile(const unsigned char* klds, const unsigned char* vlds, int key_base, int limit, float scale_log2e,
                       float logit_cap, int lane, int vc0, int k0) {
        constexpr int KCH = D / 16;
        constexpr float kRescaleThr = 8.0f;                  // log2 units: P <= 2^8 before a rescale is forced
        const bool masked = __any(key_base + k0 + NKT * 16 > limit);
        const bool capped = __builtin_amdgcn_readfirstlane(logit_cap > 0.f);
        int r = lane & 15, g = lane >> 4;
        // opaque per tile: the operand addresses below are the same for every tile of a buffer, and hoisted out of the tile loop
        // they would occupy ~50 registers beside q and the accumulator
        asm volatile("" : "+v"(r), "+v"(g));
        f32x4 s[NKT];
        // chunk (4 ks + g) ^ swz = (4 ks ^ swz[3:2] << 2) + (g ^ swz[1:0]): one pointer per 16-key tile, the k step an offset
        // (a compile-time one for the 2-bit masks)
        const unsigned char* kp[NKT];
        int khi[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int row = k0 + kt * 16 + r, sw = swz<KCH>(row);
            kp[kt] = klds + row * D + ((g ^ (sw & 3)) << 4);
            khi[kt] = sw & ~3;
        }
        // ---- S^T = K . Q^T ----
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const u32x4 kb = *reinterpret_cast<const u32x4*>(kp[kt] + (((ks * 4) ^ khi[kt]) << 4));
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(kb[0], kb[1]), qf[ks][0], s[kt], 0, 0, 0);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(kb[2], kb[3]), qf[ks][1], s[kt], 0, 0, 0);
            }
        }
        // ---- online softmax of the lane's column (attention.hip Core::tile: raw q.k in s, the scale in the exp2 argument,
        //      soft-cap and mask as wave-uniform blocks, deferred rescale) ----
        float sc = scale_log2e;
        if (capped) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = s[kt][j] * scale_log2e * 0.6931471805599453f;
                    s[kt][j] = logit_cap * tanhf(x / logit_cap) * 1.4426950408889634f;
                }
            sc = 1.f;
        }
        if (masked) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) s[kt][j] = key_base + k0 + kt * 16 + g * 4 + j < limit ? s[kt][j] : -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[kt][j]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        mx *= sc;
        float m_new = m;
        if (__any(mx > m + kRescaleThr)) {
            m_new = fmaxf(m, mx);
            const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m - m_new);
            l *= alpha;
#pragma unroll
            for (int t = 0; t < VT; ++t) o[t] *= alpha;
            m = m_new;
        }
        const float neg_m = (m_new == -INFINITY) ? 0.f : -m_new;
        float psum = 0.f;
        bf16x8 pf[NKT / 2];
#pragma unroll
        for (int ss = 0; ss < NKT / 2; ++ss) {
            u32x4 w;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                float pv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pv[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[2 * ss + a][j], sc, neg_m));   // exp2(-inf) = 0: masked keys
                    psum += pv[j];
                }
                w[2 * a] = pack_bf16x2(pv[0], pv[1]);
                w[2 * a + 1] = pack_bf16x2(pv[2], pv[3]);
            }
            pf[ss] = __builtin_bit_cast(bf16x8, w);
        }
        l += psum;     // per-lane partial; the four lane groups are summed at the end
        // ---- O^T += V^T . P: lane i of group g supplies row 32 ss + 16 (j >> 2) + 4 g + (j & 3), j = i >> 1, half i & 1 of the
        //      chunk and receives that chunk's column i at the 8 keys of P's k order ----
        constexpr int NI = VT * (NKT / 2), AHEAD = NI < 3 ? NI : 3;
        const int j = r >> 1;
        const unsigned vbase = (unsigned)(size_t)(lds_u8_ptr)vlds + (r & 1) * 8;
        // chunk (vc0 + t) ^ swz: its two low bits select one of four per-lane addresses (vc0 is a multiple of 4 when a slice has
        // four chunks or more), the rest is an offset
        unsigned va[NKT / 2][4];
        int vsw[NKT / 2];
#pragma unroll
        for (int ss = 0; ss < NKT / 2; ++ss) {
            const int row = k0 + ss * 32 + (j >> 2) * 16 + g * 4 + (j & 3);
            vsw[ss] = swz<VCH>(row);
#pragma unroll
            for (int x = 0; x < 4; ++x) va[ss][x] = vbase + row * (VCH * 16) + ((x ^ (vsw[ss] & 3)) << 4);
        }
        u32x2 vr[AHEAD + 1];
        auto rd = [&](int i) __attribute__((always_inline)) {
            const int t = i / (NKT / 2), ss = i - t * (NKT / 2);
            unsigned a;
            if constexpr (VT >= 4) a = va[ss][t & 3] + ((((vc0 + t) & ~3) ^ (vsw[ss] & ~3)) << 4);
            else a = va[ss][0] + ((((vc0 + t) ^ vsw[ss]) - (vsw[ss] & 3)) << 4);     // two-chunk slices: vc0 is even only
            asm volatile("ds_read_b64_tr_b8 %0, %1" : "=v"(vr[i % (AHEAD + 1)]) : "v"(a));
        };
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) rd(i);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            u32x2& v = vr[i % (AHEAD + 1)];
            if (i + AHEAD < NI) {
                rd(i + AHEAD);
                asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(v));
            } else if (NI - 1 - i == 2) {
                asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(v));
            } else if (NI - 1 - i == 1) {
                asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(v));
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v));
            }
            const int t = i / (NKT / 2), ss = i - t * (NKT / 2);
            o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(v[0], v[1]), pf[ss], o[t], 0, 0, 0);
        }
    }
};

// Waves = KH key groups x CT column tiles (16 q heads each) x NDV value slices; grid (request, kv head x head blocks of
// 16 CT heads, split).  Every wave keeps an online-softmax state of its own; the key halves are merged once, through LDS.
template <int D, int DV, bool V_ALIAS, int CT, int NDV, int KH>
__global__ __launch_bounds__(64 * CT * NDV * KH, 1) void decode_fp8kv_kernel(const Params p) {
    constexpr int THREADS = 64 * CT * NDV * KH;
    typedef RowDma<D, THREADS> DmaK;
    typedef RowDma<DV, THREADS> DmaV;
    static_assert(V_ALIAS || DmaV::XW == 0, "only the K image may leave half a round");
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    constexpr int KB = kKeys * D, VB = V_ALIAS ? 0 : kKeys * DV;
    constexpr int kBufs = 3 * (KB + VB) + kIdRing * kKeys * 4 <= kLdsMax ? 3 : 2;
    constexpr int DVW = DV / NDV, NKT = 4 / KH;
    constexpr int VCH = (V_ALIAS ? D : DV) / 16;
    constexpr int kDma = DmaK::FULL + (V_ALIAS ? 0 : DmaV::FULL);     // per wave and tile; + 1 for the first DmaK::XW waves
    static_assert((kBufs - 1) * (kDma + 1) <= 63, "the counted wait must fit s_waitcnt's vmcnt field");
    static_assert(KH == 1 || CT * NDV * 64 * (DVW / 4 + 2) * 4 <= kBufs * (KB + VB), "the key halves are merged in the tile buffers");

    const int b = blockIdx.x, split = blockIdx.z;
    const int group = p.HQ / p.HKV, nhb = (group + 16 * CT - 1) / (16 * CT);
    const int kvh = blockIdx.y / nhb, hb = blockIdx.y - kvh * nhb;
    const int seq_len = (int)p.b_seq_len[b];
    const int per = (seq_len + p.splits - 1) / p.splits;
    const int k_begin = split * per;
    const int k_end = (k_begin + per < seq_len) ? k_begin + per : seq_len;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kh = wave / (CT * NDV), w4 = wave - kh * (CT * NDV);
    const int ct = w4 / NDV, dsl = w4 - ct * NDV;
    const int col = (hb * CT + ct) * 16 + (lane & 15);       // q head inside the group
    const bool col_valid = col < group;
    const bool wave_active = (hb * CT + ct) * 16 < group;
    const int h = kvh * group + col;
    const bool xw = wave < DmaK::XW;                          // this wave issues the extra K round

    Core8<D, DVW, NKT> core;
    core.init();
    if (wave_active) core.load_q(col_valid ? p.q + (int64_t)b * p.q_s0 + (int64_t)h * p.q_s1 : nullptr, lane);
    const int limit = col_valid ? k_end : 0;

    const unsigned char* page = reinterpret_cast<const unsigned char*>(p.req_to_token) +
                                p.b_req_idx[b] * p.rtt_stride * (p.rtt_is64 ? 8 : 4);
    const unsigned char* kbuf = p.k_buf + (int64_t)kvh * p.kb_s1;
    const unsigned char* vbuf = p.v_buf + (int64_t)kvh * p.vb_s1;
    const int ntiles = k_end > k_begin ? (k_end - k_begin + kKeys - 1) / kKeys : 0;
    unsigned* const idring = reinterpret_cast<unsigned*>(dyn_lds + kBufs * (KB + VB));

    // id table of tile t: one 4-byte DMA per lane of wave 0 (an int64 table contributes its low words: cache rows < 2^31)
    auto lookup = [&](int t) {
        if (wave != 0) return;
        const int tt = t < ntiles ? t : ntiles - 1;          // past the end: the last tile's ids again (never used)
        const int p0 = k_begin + tt * kKeys;
        const int nk = k_end - p0 < kKeys ? k_end - p0 : kKeys;
        const int rr = lane < nk ? lane : nk - 1;
        const unsigned char* g = page + (int64_t)(p0 + rr) * (p.rtt_is64 ? 8 : 4);
        __builtin_amdgcn_global_load_lds((dma_gptr_t)g, (dma_lptr_t)(idring + (t & (kIdRing - 1)) * kKeys), 4, 0, 0);
    };
    auto issue_rows = [&](int t, unsigned char* buf) {
        const unsigned* ids = idring + (t & (kIdRing - 1)) * kKeys;
        if (p.nt) {
            DmaK::template issue<2>(buf, kbuf, p.kb_s0, ids, wave, lane);
            if constexpr (!V_ALIAS) DmaV::template issue<2>(buf + KB, vbuf, p.vb_s0, ids, wave, lane);
        } else {
            DmaK::template issue<0>(buf, kbuf, p.kb_s0, ids, wave, lane);
            if constexpr (!V_ALIAS) DmaV::template issue<0>(buf + KB, vbuf, p.vb_s0, ids, wave, lane);
        }
    };
    // Queue of a wave at the wait of tile t:  ... rows(t) | [ids(t + kBufs + 1)] rows(t+1) | [ids(t + kBufs + 2)] rows(t+2):
    // leaving the rows of the `newer` tiles outstanding covers rows(t) and the id table the rows requested after tile t need.
    auto wait_rows = [&](int newer) {
        if (newer <= 0) wait_vm<0>();
        else if (newer == 1) { if (xw) wait_vm<kDma + 1>(); else wait_vm<kDma>(); }
        else { if (xw) wait_vm<(kBufs - 1) * (kDma + 1)>(); else wait_vm<(kBufs - 1) * kDma>(); }
    };
    if (ntiles > 0) {
#pragma unroll
        for (int t = 0; t < kBufs + 2; ++t) lookup(t);
        wait_vm<0>();
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kBufs; ++t)
            if (t < ntiles) issue_rows(t, dyn_lds + t * (KB + VB));
    }
    int slot = 0;
    for (int t = 0; t < ntiles; ++t) {
        unsigned char* const cur = dyn_lds + slot * (KB + VB);
        slot = slot + 1 == kBufs ? 0 : slot + 1;
        const int left = ntiles - 1 - t;
        wait_rows(left < kBufs - 1 ? left : kBufs - 1);
        // bare s_barrier: __syncthreads()' fence would make the compiler drain vmcnt -- the rows in flight -- in front of it
        __builtin_amdgcn_s_barrier();         // every wave's share of tile t has landed, and the id table of tile t + kBufs
        asm volatile("" ::: "memory");
        if (wave_active)
            core.template tile<VCH>(cur, V_ALIAS ? cur : cur + KB, k_begin + t * kKeys, limit, p.scale_log2e, p.logit_cap, lane,
                                    dsl * (DVW / 16), kh * (NKT * 16));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();         // every wave has left `cur`
        asm volatile("" ::: "memory");
        if (t + kBufs < ntiles) {
            lookup(t + kBufs + 2);
            issue_rows(t + kBufs, cur);
        }
    }
    // ---- merge the key halves: the upper one parks {o, m, l} lane for lane in LDS (the tile buffers are dead), the lower one
    //      rescales both to the common maximum and adds ----
    float lsum = core.l;
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    constexpr int XS = DVW / 4 + 2;                     // floats per lane: its o registers, m, l
    float* xch = reinterpret_cast<float*>(dyn_lds) + (size_t)(w4 * 64 + lane) * XS;
    if (KH == 2) __syncthreads();
    if (KH == 2 && kh == 1 && wave_active) {
#pragma unroll
        for (int t = 0; t < DVW / 16; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) xch[t * 4 + j] = core.o[t][j];
        xch[DVW / 4] = core.m;
        xch[DVW / 4 + 1] = lsum;
    }
    if (KH == 2) __syncthreads();
    if (kh == 1 || !wave_active) return;
    if (KH == 2) {
        const float m1 = xch[DVW / 4], l1 = xch[DVW / 4 + 1];
        const float m0 = core.m;
        const float mt = fmaxf(m0, m1);
        // a half that saw no visible key has m = -inf and contributes nothing (and exp2(-inf - -inf) must not be taken)
        const float a0 = (m0 == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m0 - mt);
        const float a1 = (m1 == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m1 - mt);
#pragma unroll
        for (int t = 0; t < DVW / 16; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) core.o[t][j] = core.o[t][j] * a0 + xch[t * 4 + j] * a1;
        lsum = lsum * a0 + l1 * a1;
        core.m = mt;
    }
    if (!col_valid) return;
    const float inv = lsum > 0.f ? p.v_scale / lsum : 0.f;     // v_scale rides in the normalisation: the merge stays linear
    const int g4 = (lane >> 4) * 4;
    if (p.direct) {
        unsigned short* orow = p.o + (int64_t)b * p.o_s0 + (int64_t)h * p.o_s1 + dsl * DVW + g4;
#pragma unroll
        for (int t = 0; t < DVW / 16; ++t) {
            const f32x4 v = core.o[t] * inv;
            *reinterpret_cast<u32x2*>(orow + t * 16) = (u32x2){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        }
        return;
    }
    float* dst = p.logits + (((int64_t)b * p.HQ + h) * p.logit_splits + split) * (DV + 1);
#pragma unroll
    for (int t = 0; t < DVW / 16; ++t) {
        const f32x4 v = core.o[t] * inv;
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[dsl * DVW + t * 16 + g4 + j] = v[j];
    }
    // log-sum-exp of the split in log2 units (m is in log2 units); -inf marks an empty split
    if (dsl == 0 && (lane >> 4) == 0) dst[DV] = lsum > 0.f ? core.m + __builtin_amdgcn_logf(lsum) : -INFINITY;
}

// Cache write: four elements per thread, e4m3(clamp(x / scale)) with the correctly rounded fp32 division, an explicit
// clamp (a NaN stays a NaN) and v_cvt_pk_fp8_f32's round-to-nearest-even.  Aliased cache: `value` owns the first DV columns.
SGLK_DEV unsigned quant4(const unsigned short* src, float scale) {
    float x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float f = bf16_bits_to_f32(src[i]) / scale;
        x[i] = f != f ? f : fminf(fmaxf(f, -448.f), 448.f);
    }
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], w, true);
    return (unsigned)w;
}

// T rows (decode: one per request; extend: every extend token) x H heads; a row of max(D, DV) columns takes TPR threads, a
// workgroup 256 / TPR rows.
__global__ __launch_bounds__(256) void kv_cache_write_fp8_kernel(unsigned char* k_buf, int64_t kb_s0, int64_t kb_s1, unsigned char* v_buf,
                                                                 int64_t vb_s0, int64_t vb_s1, const unsigned short* key, int64_t k_s0,
                                                                 int64_t k_s1, const unsigned short* value, int64_t v_s0, int64_t v_s1,
                                                                 const void* loc, int loc_is64, int T, int D, int DV, int alias, float k_scale,
                                                                 float v_scale, int tpr) {
    const int r = threadIdx.x / tpr, x = threadIdx.x - r * tpr;
    const int64_t b = (int64_t)blockIdx.x * (256 / tpr) + r;
    const int h = blockIdx.y;
    if (r >= 256 / tpr || b >= T) return;
    const int64_t tok = loc_is64 ? reinterpret_cast<const int64_t*>(loc)[b] : (int64_t)reinterpret_cast<const int*>(loc)[b];
    for (int c = (alias ? DV : 0) + x * 4; c < D; c += tpr * 4)
        *reinterpret_cast<unsigned*>(k_buf + tok * kb_s0 + h * kb_s1 + c) = quant4(key + b * k_s0 + h * k_s1 + c, k_scale);
    for (int c = x * 4; c < DV; c += tpr * 4)
        *reinterpret_cast<unsigned*>(v_buf + tok * vb_s0 + h * vb_s1 + c) = quant4(value + b * v_s0 + h * v_s1 + c, v_scale);
}

template <int D, int DV, bool AL, int CT, int NDV, int KH>
int launch(const Params& p, dim3 grid, hipStream_t s) {
    constexpr int tile = kKeys * D + (AL ? 0 : kKeys * DV), ids = kIdRing * kKeys * 4;
    constexpr int lds = (3 * tile + ids <= kLdsMax ? 3 : 2) * tile + ids;
    SGLK_ENSURE_DYN_LDS((decode_fp8kv_kernel<D, DV, AL, CT, NDV, KH>), lds, "decode_attention_fp8kv");
    hipLaunchKernelGGL((decode_fp8kv_kernel<D, DV, AL, CT, NDV, KH>), grid, dim3(64 * CT * NDV * KH), lds, s, p);
    SGLK_CHECK_LAUNCH("decode_attention_fp8kv");
    return SGLK_OK;
}

// wide heads (D >= 256): 8 waves, 2 key halves, at most 2 column tiles;  narrow heads: 4 waves (file header)
template <int D, int DV, bool AL>
int launch_by_group(const Params& p, int B, int group, int eff, hipStream_t s) {
    constexpr bool wide = D >= 256;
    const int ct = group <= 16 ? 1 : (group <= 32 || wide) ? 2 : 4;
    const dim3 grid((unsigned)B, (unsigned)(p.HKV * ((group + 16 * ct - 1) / (16 * ct))), (unsigned)eff);
    if (ct == 1) return launch<D, DV, AL, 1, wide ? 4 : 2, 2>(p, grid, s);
    if (ct == 2) return launch<D, DV, AL, 2, wide ? 2 : 1, 2>(p, grid, s);
    if constexpr (!wide) return launch<D, DV, AL, 4, 1, 1>(p, grid, s);
    return SGLK_ERR_INVALID;
}

}  // namespace attn8
}  // namespace sglk

using namespace sglk;

int sglk::attn::launch_kv_cache_write_fp8(void* k_buf, const int64_t* kb_stride, void* v_buf, const int64_t* vb_stride, const void* key,
                                          const int64_t* key_stride, const void* value, const int64_t* value_stride, const void* loc,
                                          int loc_is64, int T, int H, int D, int DV, int alias, float k_scale, float v_scale, hipStream_t s) {
    if (T <= 0) return SGLK_OK;
    const int w = ((D > DV ? D : DV) + 3) / 4;
    const int tpr = w < 256 ? w : 256;
    hipLaunchKernelGGL(attn8::kv_cache_write_fp8_kernel, dim3((unsigned)ceil_div(T, 256 / tpr), (unsigned)H), dim3(256), 0, s,
                       (unsigned char*)k_buf, kb_stride[0], kb_stride[1], (unsigned char*)v_buf, vb_stride[0], vb_stride[1],
                       (const unsigned short*)key, key_stride[0], key_stride[1], (const unsigned short*)value, value_stride[0],
                       value_stride[1], loc, loc_is64, T, D, DV, alias, k_scale, v_scale, tpr);
    SGLK_CHECK_LAUNCH("fp8 kv cache write");
    return SGLK_OK;
}

extern "C" int sglk_decode_attention_fp8kv(const sglk_decode_attention_fp8kv_args* a, void* stream) {
    SGLK_REQUIRE(a, SGLK_ERR_INVALID, "decode_attention_fp8kv: null args");
    SGLK_REQUIRE(a->B >= 0 && a->HQ > 0 && a->HKV > 0 && a->HQ % a->HKV == 0, SGLK_ERR_INVALID,
                 "decode_attention_fp8kv: bad head counts HQ=%d HKV=%d", a->HQ, a->HKV);
    SGLK_REQUIRE(a->HQ / a->HKV <= 64, SGLK_ERR_SHAPE, "decode_attention_fp8kv: at most 64 q heads per kv head");
    SGLK_REQUIRE(a->splits > 0 && a->splits <= 64, SGLK_ERR_INVALID, "decode_attention_fp8kv: attn_logits must have 1 .. 64 splits");
    SGLK_REQUIRE(a->k_scale > 0.f && a->k_scale <= 3.0e38f && a->v_scale > 0.f && a->v_scale <= 3.0e38f, SGLK_ERR_INVALID,
                 "decode_attention_fp8kv: k_scale and v_scale must be positive and finite");
    SGLK_REQUIRE((a->D == 576 && a->DV == 512) || (a->D == 128 && a->DV == 128) || (a->D == 192 && a->DV == 128) ||
                     (a->D == 64 && a->DV == 64), SGLK_ERR_SHAPE,
                 "decode_attention_fp8kv: head dims D=%d DV=%d not built (have 576/512, 128/128, 192/128, 64/64)", a->D, a->DV);
    if (a->B == 0) return SGLK_OK;
    SGLK_REQUIRE(a->q && a->k_buffer && a->v_buffer && a->o && a->key && a->value && a->loc && a->attn_logits && a->req_to_token &&
                     a->b_req_idx && a->b_seq_len, SGLK_ERR_INVALID, "decode_attention_fp8kv: null pointer");
    SGLK_REQUIRE(a->q_stride[0] % 8 == 0 && a->q_stride[1] % 8 == 0 && ((uintptr_t)a->q % 16) == 0, SGLK_ERR_SHAPE,
                 "decode_attention_fp8kv: q rows must be 16-byte aligned");
    for (int64_t st : {a->k_buffer_stride[0], a->k_buffer_stride[1], a->v_buffer_stride[0], a->v_buffer_stride[1]})
        SGLK_REQUIRE(st % 16 == 0, SGLK_ERR_SHAPE, "decode_attention_fp8kv: cache strides must be multiples of 16 bytes");
    SGLK_REQUIRE(((uintptr_t)a->k_buffer % 16) == 0 && ((uintptr_t)a->v_buffer % 16) == 0, SGLK_ERR_SHAPE,
                 "decode_attention_fp8kv: cache base pointers must be 16-byte aligned");
    // V aliases K when it is the same storage with the same strides (MLA: v = k[..., :DV])
    const bool alias = a->v_buffer == a->k_buffer && a->v_buffer_stride[0] == a->k_buffer_stride[0] &&
                       a->v_buffer_stride[1] == a->k_buffer_stride[1] && a->DV <= a->D;
    SGLK_REQUIRE(!alias || a->k_scale == a->v_scale, SGLK_ERR_INVALID,
                 "decode_attention_fp8kv: an aliased cache needs k_scale == v_scale (one byte cannot carry two scales)");
    hipStream_t s = (hipStream_t)stream;
    int rc = attn::launch_kv_cache_write_fp8(a->k_buffer, a->k_buffer_stride, a->v_buffer, a->v_buffer_stride, a->key, a->key_stride, a->value,
                                             a->value_stride, a->loc, a->loc_is64, a->B, a->HKV, a->D, a->DV, alias ? 1 : 0, a->k_scale,
                                             a->v_scale, s);
    if (rc != SGLK_OK) return rc;
    const int eff = attn::decode_effective_splits(a->B, a->HKV, a->D, a->splits);
    attn8::Params p{};
    p.q = (const unsigned short*)a->q; p.k_buf = (const unsigned char*)a->k_buffer; p.v_buf = (const unsigned char*)a->v_buffer;
    p.q_s0 = a->q_stride[0]; p.q_s1 = a->q_stride[1]; p.kb_s0 = a->k_buffer_stride[0]; p.kb_s1 = a->k_buffer_stride[1];
    p.vb_s0 = a->v_buffer_stride[0]; p.vb_s1 = a->v_buffer_stride[1]; p.logits = a->attn_logits;
    p.req_to_token = a->req_to_token; p.rtt_stride = a->req_to_token_stride; p.rtt_is64 = a->req_to_token_is64;
    p.b_req_idx = a->b_req_idx; p.b_seq_len = a->b_seq_len; p.HQ = a->HQ; p.HKV = a->HKV;
    p.splits = eff; p.logit_splits = a->splits;
    p.scale_log2e = a->sm_scale * a->k_scale * 1.4426950408889634f;
    p.logit_cap = a->logit_cap; p.v_scale = a->v_scale;
    p.nt = knobs().dec_nt != 0 ? 1 : 0;
    p.o = (unsigned short*)a->o; p.o_s0 = a->o_stride[0]; p.o_s1 = a->o_stride[1];
    p.direct = (eff == 1 && a->o_stride[0] % 4 == 0 && a->o_stride[1] % 4 == 0 && ((uintptr_t)a->o % 8) == 0) ? 1 : 0;
    const int group = a->HQ / a->HKV;
#define DEC8_CASE(DD, DDV)                                                                                  \
    if (a->D == DD && a->DV == DDV)                                                                         \
        rc = alias ? attn8::launch_by_group<DD, DDV, true>(p, a->B, group, eff, s)                          \
                   : attn8::launch_by_group<DD, DDV, false>(p, a->B, group, eff, s);
    DEC8_CASE(576, 512)
    else DEC8_CASE(128, 128)
    else DEC8_CASE(192, 128)
    else DEC8_CASE(64, 64)
    else rc = SGLK_ERR_SHAPE;
#undef DEC8_CASE
    if (rc != SGLK_OK || p.direct) return rc;
    return attn::launch_decode_merge(a->attn_logits, a->o, a->o_stride[0], a->o_stride[1], a->B, a->HQ, eff, a->splits, a->DV, s);
}
