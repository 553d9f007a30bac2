// Pieces of attention.hip that the fp8-cache forms (attention_fp8kv.hip, attention_extend_fp8kv.hip) use too.
#pragma once
#include "sglk_common.h"
#include "knobs.h"

namespace sglk {
namespace attn {

// KV splits decode attention uses out of the `splits` the caller's attn_logits scratch has room for (see the definition)
int decode_effective_splits(int B, int HKV, int D, int splits);

// combines the first `eff` per-split partials (O / l, log-sum-exp) of attn_logits [B][HQ][splits][DV + 1] into o (bf16)
int launch_decode_merge(const float* attn_logits, void* o, int64_t o_s0, int64_t o_s1, int B, int HQ, int eff, int splits, int DV,
                        hipStream_t stream);

// kv_cache_write_kernel (attention.hip) over T rows x H heads: k_buf[loc[t]][h] = key[t][h], v_buf likewise, bit-exact; strides
// {token, head} in elements.  V after K in program order: with an aliased cache `value` wins in the first DV columns.
int launch_kv_cache_write(void* k_buf, const int64_t* kb_stride, void* v_buf, const int64_t* vb_stride, const void* key,
                          const int64_t* key_stride, const void* value, const int64_t* value_stride, const void* loc, int loc_is64,
                          int T, int H, int D, int DV, hipStream_t stream);

// quantising write of the fp8-cache operators (attention_fp8kv.hip): k_buf[loc[t]][h] = e4m3(clamp(key[t][h] / k_scale, +-448)) for
// T rows x H heads, v_buf likewise; cache strides {token, head} in bytes, key / value strides in elements
int launch_kv_cache_write_fp8(void* k_buf, const int64_t* kb_stride, void* v_buf, const int64_t* vb_stride, const void* key,
                              const int64_t* key_stride, const void* value, const int64_t* value_stride, const void* loc, int loc_is64,
                              int T, int H, int D, int DV, int alias, float k_scale, float v_scale, hipStream_t stream);

// ---- device pieces of extend attention (attention.hip) that the fp8-cache form (attention_extend_fp8kv.hip) builds on too ----
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

constexpr int kKeys = 64;   // keys per tile

template <int CHUNKS>
struct Swz {   // XOR mask for 16-byte chunks of a row with CHUNKS chunks (mask+1 must divide CHUNKS)
    // a ds_read_b128 is serviced in groups of SIXTEEN lanes ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH.md 'LDS'), i.e. 16 rows of
    // two neighbouring chunk columns in the K-fragment read: only a 4-bit mask spreads those over all 64 banks (with 3 bits the
    // two columns share one 128-byte window: a 2-way conflict on every fragment read).  Rows whose chunk count is not a multiple
    // of 16 (D = 192, 576) keep the 3-bit mask.
    static constexpr int mask = (CHUNKS % 16 == 0) ? 15 : ((CHUNKS % 8 == 0) ? 7 : ((CHUNKS % 4 == 0) ? 3 : ((CHUNKS % 2 == 0) ? 1 : 0)));
};

struct KvSource {
    // key position p of the stream -> row pointer.  p < n_paged: buf + page[p] * stride_tok;  else ext + (p - n_paged) * ext_stride_tok
    const unsigned short* buf;
    int64_t buf_stride_tok;
    const void* page;     // int32 or int64 token ids
    int page_is64;
    int n_paged;
    const unsigned short* ext;
    int64_t ext_stride_tok;
};

SGLK_DEV const unsigned short* kv_row(const KvSource& s, int p) {
    if (p < s.n_paged) {
        const int64_t tok = s.page_is64 ? reinterpret_cast<const int64_t*>(s.page)[p] : (int64_t)reinterpret_cast<const int*>(s.page)[p];
        return s.buf + tok * s.buf_stride_tok;
    }
    return s.ext + (int64_t)(p - s.n_paged) * s.ext_stride_tok;
}
// Every position is paged (decode).  Branch-free on purpose: a branch around the page lookup makes the compiler wait
// for every lookup before the next one is issued, which serialises a tile's 4..18 row fetches per lane (measured:
// 13.6 us per 64-key MLA tile instead of ~3).
SGLK_DEV const unsigned short* kv_row_paged(const KvSource& s, int p) {
    const int64_t tok = s.page_is64 ? reinterpret_cast<const int64_t*>(s.page)[p] : (int64_t)reinterpret_cast<const int*>(s.page)[p];
    return s.buf + tok * s.buf_stride_tok;
}

// stage `nkeys` (<= 64) rows of WIDTH bf16 into the swizzled LDS image; missing rows are zero-filled
template <int WIDTH, int THREADS>
SGLK_DEV void stage_tile(unsigned char* lds, const KvSource& src, int p0, int nkeys, const unsigned short** rowptr_lds) {
    constexpr int CH = WIDTH / 8;
    constexpr int MASK = Swz<CH>::mask;
    if (threadIdx.x < kKeys) rowptr_lds[threadIdx.x] = threadIdx.x < nkeys ? kv_row(src, p0 + threadIdx.x) : nullptr;
    __syncthreads();
    for (int c = threadIdx.x; c < kKeys * CH; c += THREADS) {
        const int row = c / CH, ch = c - row * CH;
        const unsigned short* rp = rowptr_lds[row];
        uint4 v = make_uint4(0, 0, 0, 0);
        if (rp) v = *reinterpret_cast<const uint4*>(rp + ch * 8);
        *reinterpret_cast<uint4*>(lds + row * (WIDTH * 2) + ((ch ^ (row & MASK)) << 4)) = v;
    }
}

// Split staging for software pipelining (issue the global loads of tile i+1 before computing tile i, write them to the
// other LDS buffer afterwards).  Every thread resolves the rows of its own chunks (page lookups hit L1), so no
// row-pointer table and no extra barrier is needed.  NCH = chunks per thread.
template <int WIDTH, int THREADS>
struct TileRegs {
    static constexpr int CH = WIDTH / 8;
    static constexpr int NCH = (kKeys * CH + THREADS - 1) / THREADS;
    uint4 v[NCH];
    // real_w: valid elements per row (<= WIDTH, even; the image is zero-padded beyond it); aligned: rows and their
    // 8-element chunks are 16-byte aligned (else the chunk is gathered as four dwords)
    SGLK_DEV void load(const KvSource& src, int p0, int nkeys, int real_w = WIDTH, bool aligned = true) {
        // two passes: row pointers (page lookups) first, then the row loads back to back
        const unsigned short* rp[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = threadIdx.x + i * THREADS;
            const int row = c / CH, ch = c - row * CH;
            rp[i] = (c < kKeys * CH && row < nkeys && ch * 8 < real_w) ? kv_row(src, p0 + row) + ch * 8 : nullptr;
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            v[i] = make_uint4(0, 0, 0, 0);
            if (!rp[i]) continue;
            const int ch = (threadIdx.x + i * THREADS) % CH;
            if (aligned && ch * 8 + 8 <= real_w) {
                v[i] = *reinterpret_cast<const uint4*>(rp[i]);
            } else {
                const unsigned* d = reinterpret_cast<const unsigned*>(rp[i]);
                const int left = real_w - ch * 8;            // 2, 4, 6 or >= 8 valid elements
                v[i].x = d[0];
                if (left > 2) v[i].y = d[1];
                if (left > 4) v[i].z = d[2];
                if (left > 6) v[i].w = d[3];
            }
        }
    }
    SGLK_DEV void store(unsigned char* lds) const {
        constexpr int MASK = Swz<CH>::mask;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = threadIdx.x + i * THREADS;
            const int row = c / CH, ch = c - row * CH;
            if (c < kKeys * CH) *reinterpret_cast<uint4*>(lds + row * (WIDTH * 2) + ((ch ^ (row & MASK)) << 4)) = v[i];
        }
    }
};

// Per-wave attention state and the per-tile update.  D, DV: head dims of K and V; QT: 16-column query tiles.
template <int D, int DV, int QT>
struct Core {
    static constexpr int KS = D / 32;       // k-steps of Q.K
    static constexpr int VT = DV / 16;      // output tiles
    static constexpr int KCH = D / 8, VCH = DV / 8;

    bf16x8 qf[QT][KS];
    f32x4 o[QT][VT];
    float m[QT], l[QT];

    SGLK_DEV void init() {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            m[qt] = -INFINITY;
            l[qt] = 0.f;
#pragma unroll
            for (int t = 0; t < VT; ++t) o[qt][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    // column qt*16 + (lane&15) reads its query row (nullptr = padding column)
    // d_real: valid elements of the row (multiple of 8, <= D; zero beyond)
    SGLK_DEV void load_q(int qt, const unsigned short* qrow, int lane, int d_real = D) {
        const int g = lane >> 4;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (qrow && ks * 32 + g * 8 < d_real) v = *reinterpret_cast<const uint4*>(qrow + ks * 32 + g * 8);
            qf[qt][ks] = __builtin_bit_cast(bf16x8, v);
        }
    }

    // one 64-key tile.  key_base: stream position of the tile's first key; limit[qt]: the lane's column may see keys
    // with position < limit; V_ALIAS: V rows live in the K image (row width D), else in its own image (row width DV)
    // DV here is the width of the V slice this wave accumulates; dv0 = its first column inside the V image, whose rows
    // are VROW elements wide (0 = DV, i.e. the wave owns the whole width)
    // NKT = 16-key tiles this wave takes from the image (4 = all 64 keys; 2 = the 32 keys from row k0, decode kernel)
    // ASM_TR: the transposed V reads are inline asm with hand-counted lgkmcnt waits.  The compiler does not know what the
    // ds_read_tr builtin may alias and puts an s_waitcnt vmcnt(0) in front of the first one whenever LDS-DMA writes are pending:
    // in the decode kernel that drained the NEXT tiles' rows in the middle of every tile.
    template <bool V_ALIAS, int VROW = 0, int NKT = 4, bool ASM_TR = false>
    SGLK_DEV void tile(const unsigned char* klds, const unsigned char* vlds, int key_base, const int (&limit)[QT],
                       float scale_log2e, float logit_cap, int lane, int dv0 = 0, int k0 = 0) {
        int lim_min = limit[0];
#pragma unroll
        for (int qt = 1; qt < QT; ++qt) lim_min = limit[qt] < lim_min ? limit[qt] : lim_min;
        const bool masked = __any(key_base + k0 + NKT * 16 > lim_min);
        const bool capped = __builtin_amdgcn_readfirstlane(logit_cap > 0.f);
        constexpr int KMASK = Swz<KCH>::mask;
        constexpr int VW = V_ALIAS ? D : (VROW ? VROW : DV);   // row width of the image V is read from
        constexpr int VMASK = V_ALIAS ? KMASK : Swz<VW / 8>::mask;
        constexpr float kRescaleThr = 8.0f;                  // log2 units: P <= 2^8 before a rescale is forced
        const int r = lane & 15, g = lane >> 4;
        f32x4 s[QT][NKT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) s[qt][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // ---- S^T = K . Q^T ----
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const int row = k0 + kt * 16 + r;
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(klds + row * (D * 2) + (((ks * 4 + g) ^ (row & KMASK)) << 4));
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
                    s[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][ks], s[qt][kt], 0, 0, 0);
            }
        }
        // ---- online softmax per column (lane) ----
        bf16x8 pf[QT][NKT / 2];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            // s holds RAW q.k; the softmax scale rides in the exp2 argument (one v_fma per element instead of a
            // multiply and a subtract).  The soft-cap and the visibility mask are whole wave-uniform blocks (one
            // scalar branch each), so full tiles below the causal diagonal run neither.
            float sc = scale_log2e;
            if (capped) {
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // cap * tanh(x / cap) on the natural-log-scale logit, stored in log2 units
                        const float x = s[qt][kt][j] * scale_log2e * 0.6931471805599453f;
                        s[qt][kt][j] = logit_cap * tanhf(x / logit_cap) * 1.4426950408889634f;
                    }
                sc = 1.f;
            }
            if (masked) {
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int key = key_base + k0 + kt * 16 + g * 4 + j;
                        s[qt][kt][j] = key < limit[qt] ? s[qt][kt][j] : -INFINITY;
                    }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[qt][kt][j]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            mx *= sc;                                        // log2 units (sc > 0)
            // Deferred rescale: keep the old reference maximum while the new one is at most 2^thr above it (P stays
            // <= 2^thr, harmless in fp32 sums and in bf16 P); the branch is wave-uniform.  The first tile (m = -inf)
            // and any larger jump take the exact path.
            float m_new = m[qt];
            if (__any(mx > m[qt] + kRescaleThr)) {
                m_new = fmaxf(m[qt], mx);
                const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m[qt] - m_new);
                l[qt] *= alpha;
#pragma unroll
                for (int t = 0; t < VT; ++t) o[qt][t] *= alpha;
                m[qt] = m_new;
            }
            const float neg_m = (m_new == -INFINITY) ? 0.f : -m_new;
            float psum = 0.f;
            float p[NKT][4];
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    p[kt][j] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[qt][kt][j], sc, neg_m));   // exp2(-inf) = 0 for masked keys
                    psum += p[kt][j];
                }
            l[qt] += psum;     // per-lane partial (this lane's keys); lane groups are summed at the end
#pragma unroll
            for (int ss = 0; ss < NKT / 2; ++ss) {
                u32x4 w;
                w[0] = pack_bf16x2(p[2 * ss][0], p[2 * ss][1]);
                w[1] = pack_bf16x2(p[2 * ss][2], p[2 * ss][3]);
                w[2] = pack_bf16x2(p[2 * ss + 1][0], p[2 * ss + 1][1]);
                w[3] = pack_bf16x2(p[2 * ss + 1][2], p[2 * ss + 1][3]);
                pf[qt][ss] = __builtin_bit_cast(bf16x8, w);
            }
        }
        // ---- O^T += V^T . P ----
        const int q = r >> 2, pp = r & 3;   // transposed read: lane supplies row q, columns 4pp.. of its group's 4x16 block
        if constexpr (ASM_TR) {
            typedef __attribute__((ext_vector_type(8))) short s16x8;
            constexpr int NI = VT * (NKT / 2);
            s16x4 lo[2], hi[2];
            auto rd = [&](int i, s16x4& l, s16x4& h) {
                const int t = i / (NKT / 2), ss = i - t * (NKT / 2);
                const int row0 = k0 + ss * 32 + g * 4 + q, row1 = row0 + 16;
                const int col = dv0 + t * 16 + pp * 4;
                const int ch = col >> 3, sub = (col & 7) * 2;
                const unsigned a0 = (unsigned)(size_t)(lds_s16x4_ptr)(vlds + row0 * (VW * 2) + ((ch ^ (row0 & VMASK)) << 4) + sub);
                const unsigned a1 = (unsigned)(size_t)(lds_s16x4_ptr)(vlds + row1 * (VW * 2) + ((ch ^ (row1 & VMASK)) << 4) + sub);
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(l) : "v"(a0));
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(h) : "v"(a1));
            };
            rd(0, lo[0], hi[0]);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                s16x4& l = lo[i & 1];
                s16x4& h = hi[i & 1];
                if (i + 1 < NI) {
                    rd(i + 1, lo[(i + 1) & 1], hi[(i + 1) & 1]);
                    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(l), "+v"(h));     // all but the two reads just issued
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(l), "+v"(h));
                }
                s16x8 vv;
                vv[0] = l[0]; vv[1] = l[1]; vv[2] = l[2]; vv[3] = l[3];
                vv[4] = h[0]; vv[5] = h[1]; vv[6] = h[2]; vv[7] = h[3];
                const bf16x8 vf = __builtin_bit_cast(bf16x8, vv);
                const int t = i / (NKT / 2), ss = i - t * (NKT / 2);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
                    o[qt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt][ss], o[qt][t], 0, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int t = 0; t < VT; ++t) {
#pragma unroll
            for (int ss = 0; ss < NKT / 2; ++ss) {
                const int row0 = k0 + ss * 32 + g * 4 + q;
                const int row1 = row0 + 16;
                const int col = dv0 + t * 16 + pp * 4;      // in elements; 4 elements = 8 bytes inside one 16-B chunk
                const int ch = col >> 3, sub = (col & 7) * 2;
                const unsigned char* a0 = vlds + row0 * (VW * 2) + ((ch ^ (row0 & VMASK)) << 4) + sub;
                const unsigned char* a1 = vlds + row1 * (VW * 2) + ((ch ^ (row1 & VMASK)) << 4) + sub;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(a0));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(a1));
                typedef __attribute__((ext_vector_type(8))) short s16x8;
                s16x8 vv;
                vv[0] = lo[0]; vv[1] = lo[1]; vv[2] = lo[2]; vv[3] = lo[3];
                vv[4] = hi[0]; vv[5] = hi[1]; vv[6] = hi[2]; vv[7] = hi[3];
                const bf16x8 vf = __builtin_bit_cast(bf16x8, vv);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
                    o[qt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt][ss], o[qt][t], 0, 0, 0);
            }
        }
    }

    // total of the per-lane partial sums of a column (the 4 lane groups hold disjoint keys)
    SGLK_DEV float column_sum(int qt) const {
        float v = l[qt];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        return v;
    }
};

struct ExtendParams {
    const unsigned short *q, *k_ext, *v_ext, *k_buf, *v_buf;
    unsigned short* o;
    int64_t q_s0, q_s1, ke_s0, ke_s1, ve_s0, ve_s1, kb_s0, kb_s1, vb_s0, vb_s1, o_s0, o_s1;   // element strides [token][head]
    const void* req_to_tokens;   // [B][L]
    int64_t rtt_stride;
    int rtt_is64;
    const int64_t* b_req_idx;
    const int64_t* b_seq_len;
    const int* b_seq_len_extend;
    const int* b_start_loc_extend;
    int HQ, HKV, HBUF;
    float sm_scale, logit_cap;
    // flash_attn_varlen_func form (/root/reference/test_flash_attn_varlen.py:100-108): no paged prefix, queries and keys of
    // sequence b are rows cu_q[b]..cu_q[b+1] of q / cu_k[b]..cu_k[b+1] of k_ext, v_ext; causal = top-left aligned mask
    int varlen, causal;
    const int* cu_q;
    const int* cu_k;
    int d_real, dv_real;     // head dims of the tensors; the kernel's D / DV are these rounded up (zero-padded images)
    int v_aligned;           // V rows / chunks are 16-byte aligned
    int B, nqblk, n_cu, order, pair;   // launch geometry (see the kernel's workgroup-id decomposition)
};

inline int attn_cus() { return device_cu_count(); }
inline int attn_order(int dflt) {   // A/B override: bit 0 = flip second wave, bit 1 = heads fastest
    return knobs().attn_order >= 0 ? knobs().attn_order : dflt;
}

// heavy + light query blocks in one workgroup (see the kernel): SGLK_ATTN_PAIR = 0 / 1 overrides
inline int pair_blocks(int nqblk, int64_t wgs_unpaired, int n_cu, int causal) {
    if (nqblk < 2 || !causal) return 0;
    if (knobs().attn_pair >= 0) return knobs().attn_pair;
    return wgs_unpaired <= 2 * (int64_t)n_cu ? 1 : 0;
}

typedef const __attribute__((address_space(1))) void* dma_gptr_t;
typedef __attribute__((address_space(3))) void* dma_lptr_t;

// A group's half of a 64-row tile by LDS-DMA: 256 threads x 2 instructions of 16 bytes per lane, no registers, no ds_write.
// The image is linear per wave (1 KiB per instruction), so the XOR swizzle is applied to the SOURCE chunk a lane fetches.
// Rows past `nkeys` repeat the last real row (finite data: their probabilities are exactly 0).
// V image of the two-phase kernel (16 chunks per row): chunk c of row r sits in slot c ^ vswz(r).  A ds_read_b64_tr_b16 of 32
// lanes takes a 32-byte column pair from 8 consecutive rows; with the K image's 3-bit mask those fall into one 128-byte window
// (half the banks, two passes), with the row number in bits 3:1 they cover all 64 banks.
SGLK_DEV int vswz(int row) { return ((row & 7) << 1) | ((row >> 3) & 1); }

template <int WIDTH, int FORM, bool VIMG = false>
struct HalfDma {
    static constexpr int CH = WIDTH / 8;
    static constexpr int N = CH / 8;                 // instructions per thread: a group's 32 rows x CH chunks over 256 threads
    static_assert(CH % 8 == 0, "row width must be a multiple of 64 elements");
    const unsigned short* g[N];
    SGLK_DEV void prep(const KvSource& src, int p0, int nkeys, int grp, int t256) {
        constexpr int MASK = Swz<CH>::mask;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int c = grp * (32 * CH) + i * 256 + t256;
            const int row = c / CH, slot = c - row * CH;
            const int rr = row < nkeys ? row : nkeys - 1;
            const int pos = p0 + rr;
            const unsigned short* base;
            if (FORM == 0) {
                const int pi = pos < src.n_paged ? pos : 0;
                int64_t tok = 0;
                if (src.n_paged > 0)
                    tok = src.page_is64 ? reinterpret_cast<const int64_t*>(src.page)[pi] : (int64_t)reinterpret_cast<const int*>(src.page)[pi];
                const unsigned short* a = src.buf + tok * src.buf_stride_tok;
                const unsigned short* b = src.ext + (int64_t)(pos - src.n_paged) * src.ext_stride_tok;
                base = pos < src.n_paged ? a : b;
            } else {
                base = src.ext + (int64_t)pos * src.ext_stride_tok;
            }
            g[i] = base + ((slot ^ (VIMG ? vswz(row) : (row & MASK))) << 3);
        }
    }
    SGLK_DEV void issue(unsigned char* lds, int grp, int wv) const {
#pragma unroll
        for (int i = 0; i < N; ++i)
            __builtin_amdgcn_global_load_lds((dma_gptr_t)g[i], (dma_lptr_t)(lds + (grp * (32 * CH) + i * 256 + wv * 64) * 16), 16, 0, 0);
    }
};

// A/B knobs of the decode kernel (compile time): images up to this size are double buffered; wave groups for wide heads
#ifndef SGLK_DEC_DOUBLE_LIMIT
#define SGLK_DEC_DOUBLE_LIMIT (150 * 1024)
#endif
#ifndef SGLK_DEC_KH_WIDE
#define SGLK_DEC_KH_WIDE 2
#endif

// LDS-DMA staging of one 64-key tile (no registers, asynchronous): the image is written linearly, 1 KiB per wave
// instruction, and the 16-byte-chunk swizzle is applied to the SOURCE address.  Rows past `nkeys` re-read the last valid
// row (finite data: their probabilities are exactly 0, but 0 * garbage must not be NaN).  Returns nothing to wait on:
// the caller counts the instructions (kDmaPerThread) in its s_waitcnt vmcnt.
template <int WIDTH, int THREADS>   // THREADS = the decode kernel's workgroup size (256 or 512)
struct TileDma {
    static constexpr int CH = WIDTH / 8;
    static constexpr int N = (kKeys * CH + THREADS - 1) / THREADS;   // DMA instructions per wave per tile
    static_assert((kKeys * CH) % THREADS == 0, "the image must be a whole number of workgroup-wide DMA rounds");
    // Decode kernel: the cache rows (page-table entries) of a tile are themselves fetched by LDS-DMA -- ONE 256-byte instruction of
    // one wave per tile, into a small ring of id tables -- a whole step before the tile's rows are requested, and the row
    // requests read them from LDS.  (Per-lane lookups cost N loads and N registers per lane and tile; and loads retire in order,
    // so a lookup queued behind the previous tile's rows could not be consumed before those had landed.)  Positions past `nkeys`
    // repeat the last valid row.  An int64 table contributes its low words (cache rows are < 2^31).
    SGLK_DEV static void lookup_dma(unsigned* ids, const KvSource& src, int p0, int nkeys, int lane) {
        const int rr = lane < nkeys ? lane : nkeys - 1;
        const unsigned char* g = reinterpret_cast<const unsigned char*>(src.page) + (int64_t)(p0 + rr) * (src.page_is64 ? 8 : 4);
        __builtin_amdgcn_global_load_lds((dma_gptr_t)g, (dma_lptr_t)ids, 4, 0, 0);
    }
    template <int AUX>   // 2 = non-temporal: rows that one workgroup reads once need not stay in L2 / the Infinity Cache
    SGLK_DEV static void issue_rows(unsigned char* lds, const KvSource& src, const unsigned* ids, int wave, int lane) {
        constexpr int MASK = Swz<CH>::mask;
        int tok[N];
#pragma unroll
        for (int i = 0; i < N; ++i) tok[i] = (int)ids[(i * THREADS + wave * 64 + lane) / CH];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int c = i * THREADS + wave * 64 + lane;
            const int row = c / CH, slot = c - row * CH;
            const unsigned short* g = src.buf + (int64_t)tok[i] * src.buf_stride_tok + ((slot ^ (row & MASK)) << 3);
            __builtin_amdgcn_global_load_lds((dma_gptr_t)g, (dma_lptr_t)(lds + (i * THREADS + wave * 64) * 16), 16, 0, AUX);
        }
    }
    SGLK_DEV static void issue(unsigned char* lds, const KvSource& src, int p0, int nkeys, int wave, int lane) {
        constexpr int MASK = Swz<CH>::mask;
        constexpr int HALF = (N + 1) / 2;
        // two passes per half: all row lookups first (independent loads, one wait), then the DMA instructions
#pragma unroll
        for (int h0 = 0; h0 < N; h0 += HALF) {
            const unsigned short* g[HALF];
#pragma unroll
            for (int j = 0; j < HALF; ++j) {
                const int i = h0 + j;
                if (i < N) {
                    const int c = i * THREADS + wave * 64 + lane;        // linear chunk of the image this lane fills
                    const int row = c / CH, slot = c - row * CH;
                    const int rr = row < nkeys ? row : nkeys - 1;
                    g[j] = kv_row_paged(src, p0 + rr) + ((slot ^ (row & MASK)) << 3);
                }
            }
#pragma unroll
            for (int j = 0; j < HALF; ++j) {
                const int i = h0 + j;
                if (i < N)
                    __builtin_amdgcn_global_load_lds((dma_gptr_t)g[j], (dma_lptr_t)(lds + (i * THREADS + wave * 64) * 16), 16, 0, 0);
            }
        }
    }
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
// max over the lanes l ^ 16 / l ^ 32 by row swaps (gfx950 v_permlane16_swap / v_permlane32_swap): with both operands the same
// register the two results hold the two rows of every pair in all lanes of the pair
SGLK_DEV float xor16_max(float v) {
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    return fmaxf(__builtin_bit_cast(float, r[0]), __builtin_bit_cast(float, r[1]));
}
SGLK_DEV float xor32_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    return fmaxf(__builtin_bit_cast(float, r[0]), __builtin_bit_cast(float, r[1]));
}

#ifndef SGLK_PP_AHEAD
#define SGLK_PP_AHEAD 4
#endif
#ifndef SGLK_PP_AHEAD_192
#define SGLK_PP_AHEAD_192 2
#endif
template <int D_, int AHEAD = SGLK_PP_AHEAD>
struct CorePP {
    static constexpr int D = D_, DV = 128, QT = 2, KS = D_ / 32, VT = 8, NKT = 4;
    static constexpr int kAhead = AHEAD;   // operand fragments (16 bytes per lane) in flight ahead of the MFMAs
    bf16x8 qf[QT][KS];
    f32x4 o[QT][VT];
    f32x4 s[QT][NKT];
    bf16x8 pf[QT][NKT / 2];
    float m[QT], l[QT];

    SGLK_DEV void init() {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            m[qt] = -INFINITY;
            l[qt] = 0.f;
#pragma unroll
            for (int t = 0; t < VT; ++t) o[qt][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    SGLK_DEV void load_q(int qt, const unsigned short* qrow, int lane) {
        const int g = lane >> 4;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (qrow) v = *reinterpret_cast<const uint4*>(qrow + ks * 32 + g * 8);
            qf[qt][ks] = __builtin_bit_cast(bf16x8, v);
        }
    }
    // S^T = K . Q^T of one 64-key tile.  Only ONE wave of a SIMD is in its matrix slot, so nothing else hides the LDS latency of
    // the operand reads: they are issued eight fragments ahead of the MFMAs that consume them (scheduling fences pin the order;
    // left alone the scheduler keeps one read in flight and every pair of MFMAs waits a full LDS round trip).
    SGLK_DEV void qk(const unsigned char* klds, int lane) {
        constexpr int KMASK = Swz<D / 8>::mask;
        const int r = lane & 15, g = lane >> 4;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) s[qt][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        bf16x8 kf[KS * NKT];
#pragma unroll
        for (int i = 0; i < KS * NKT; ++i) {
            const int ks = i / NKT, kt = i % NKT;
            const int row = kt * 16 + r;
#if (SGLK_PP_ABL & 4)       // timing ablation 4: no operand reads
            kf[i] = qf[0][ks];
            (void)row;
#else
            kf[i] = *reinterpret_cast<const bf16x8*>(klds + row * (D * 2) + (((ks * 4 + g) ^ (row & KMASK)) << 4));
#endif
        }
#pragma unroll
        for (int i = 0; i < KS * NKT; ++i) {
            const int ks = i / NKT, kt = i % NKT;
#pragma unroll
#if (SGLK_PP_ABL & 8)       // timing ablation 8: no MFMAs (the reads stay)
            asm volatile("" ::"v"(kf[i]));
            (void)ks; (void)kt;
#else
            for (int qt = 0; qt < QT; ++qt)
                s[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[i], qf[qt][ks], s[qt][kt], 0, 0, 0);
#endif
        }
        __builtin_amdgcn_sched_group_barrier(0x100, kAhead, 0);
#pragma unroll
        for (int i = 0; i < KS * NKT - kAhead; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
#pragma unroll
        for (int i = 0; i < kAhead; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    }
    // online softmax of the tile in `s` -> `pf` (same arithmetic as Core::tile)
    SGLK_DEV void softmax(int key_base, const int (&limit)[QT], float scale_log2e, float logit_cap, int lane) {
#if (SGLK_PP_ABL & 1)     // timing ablation: no softmax arithmetic (wrong results)
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int ss = 0; ss < NKT / 2; ++ss) {
                u32x4 w;
                w[0] = pack_bf16x2(s[qt][2 * ss][0], s[qt][2 * ss][1]);
                w[1] = pack_bf16x2(s[qt][2 * ss][2], s[qt][2 * ss][3]);
                w[2] = pack_bf16x2(s[qt][2 * ss + 1][0], s[qt][2 * ss + 1][1]);
                w[3] = pack_bf16x2(s[qt][2 * ss + 1][2], s[qt][2 * ss + 1][3]);
                pf[qt][ss] = __builtin_bit_cast(bf16x8, w);
            }
        return;
#endif
        int lim_min = limit[0] < limit[1] ? limit[0] : limit[1];
        const bool masked = __any(key_base + NKT * 16 > lim_min);
        const bool capped = __builtin_amdgcn_readfirstlane(logit_cap > 0.f);
        constexpr float kRescaleThr = 8.0f;
        const int g = lane >> 4;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            float sc = scale_log2e;
            if (capped) {
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float x = s[qt][kt][j] * scale_log2e * 0.6931471805599453f;
                        s[qt][kt][j] = logit_cap * tanhf(x / logit_cap) * 1.4426950408889634f;
                    }
                sc = 1.f;
            }
            if (masked) {
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int key = key_base + kt * 16 + g * 4 + j;
                        s[qt][kt][j] = key < limit[qt] ? s[qt][kt][j] : -INFINITY;
                    }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[qt][kt][j]);
            // the column's four lane groups: row swaps on the VALU (no LDS round trip -- this wave is alone on its SIMD's VALU
            // during the slot, nothing would hide a ds_bpermute's latency)
            mx = xor16_max(mx);
            mx = xor32_max(mx);
            mx *= sc;
            float m_new = m[qt];
            if (__any(mx > m[qt] + kRescaleThr)) {
                m_new = fmaxf(m[qt], mx);
                const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m[qt] - m_new);
                l[qt] *= alpha;
#pragma unroll
                for (int t = 0; t < VT; ++t) o[qt][t] *= alpha;
                m[qt] = m_new;
            }
            const float neg_m = (m_new == -INFINITY) ? 0.f : -m_new;
            // packed fp32 (v_pk_fma_f32 / v_pk_add_f32: two elements per instruction)
            const f32x2 sc2 = {sc, sc}, nm2 = {neg_m, neg_m};
            f32x2 ps = {0.f, 0.f};
            float pr[NKT][4];
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const f32x2 lo = {s[qt][kt][0], s[qt][kt][1]}, hi = {s[qt][kt][2], s[qt][kt][3]};
                const f32x2 y0 = __builtin_elementwise_fma(lo, sc2, nm2), y1 = __builtin_elementwise_fma(hi, sc2, nm2);
                const f32x2 e0 = {__builtin_amdgcn_exp2f(y0[0]), __builtin_amdgcn_exp2f(y0[1])};   // exp2(-inf) = 0 for masked keys
                const f32x2 e1 = {__builtin_amdgcn_exp2f(y1[0]), __builtin_amdgcn_exp2f(y1[1])};
                ps += e0;
                ps += e1;
                pr[kt][0] = e0[0]; pr[kt][1] = e0[1]; pr[kt][2] = e1[0]; pr[kt][3] = e1[1];
            }
            l[qt] += ps[0] + ps[1];
#pragma unroll
            for (int ss = 0; ss < NKT / 2; ++ss) {
                u32x4 w;
                w[0] = pack_bf16x2(pr[2 * ss][0], pr[2 * ss][1]);
                w[1] = pack_bf16x2(pr[2 * ss][2], pr[2 * ss][3]);
                w[2] = pack_bf16x2(pr[2 * ss + 1][0], pr[2 * ss + 1][1]);
                w[3] = pack_bf16x2(pr[2 * ss + 1][2], pr[2 * ss + 1][3]);
                pf[qt][ss] = __builtin_bit_cast(bf16x8, w);
            }
        }
    }
    // O^T += V^T . P  (operand reads eight ahead, as in qk)
    SGLK_DEV void pv(const unsigned char* vlds, int lane) {
        const int r = lane & 15, g = lane >> 4;
        const int q = r >> 2, pp = r & 3;
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        s16x4 lo[VT * 2], hi[VT * 2];
#pragma unroll
        for (int i = 0; i < VT * 2; ++i) {
            const int t = i >> 1, ss = i & 1;
            const int row0 = ss * 32 + g * 4 + q;
            const int row1 = row0 + 16;
            const int col = t * 16 + pp * 4;
            const int ch = col >> 3, sub = (col & 7) * 2;
            const unsigned char* a0 = vlds + row0 * (DV * 2) + ((ch ^ vswz(row0)) << 4) + sub;
            const unsigned char* a1 = vlds + row1 * (DV * 2) + ((ch ^ vswz(row1)) << 4) + sub;
#if (SGLK_PP_ABL & 4)
            lo[i] = __builtin_bit_cast(s16x4, (uint2){(unsigned)i, 0u});
            hi[i] = lo[i];
            (void)a0; (void)a1;
#else
            lo[i] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(a0));
            hi[i] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(a1));
#endif
        }
#pragma unroll
        for (int i = 0; i < VT * 2; ++i) {
            const int t = i >> 1, ss = i & 1;
            s16x8 vv;
            vv[0] = lo[i][0]; vv[1] = lo[i][1]; vv[2] = lo[i][2]; vv[3] = lo[i][3];
            vv[4] = hi[i][0]; vv[5] = hi[i][1]; vv[6] = hi[i][2]; vv[7] = hi[i][3];
            const bf16x8 vf = __builtin_bit_cast(bf16x8, vv);
#if (SGLK_PP_ABL & 8)
            asm volatile("" ::"v"(vf));
            (void)t; (void)ss;
#else
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
                o[qt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt][ss], o[qt][t], 0, 0, 0);
#endif
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * kAhead, 0);
#pragma unroll
        for (int i = 0; i < 16 - kAhead; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
#pragma unroll
        for (int i = 0; i < kAhead; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    }
    SGLK_DEV float column_sum(int qt) const {
        float v = l[qt];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        return v;
    }
};

// end of a slot: LDS writes of this wave have landed (lgkmcnt(0)); the staged global loads stay in flight across the barrier
// (__syncthreads would wait for them -- a slot would then last at least one memory round trip)
SGLK_DEV void slot_barrier_m() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);     // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
SGLK_DEV void slot_barrier_v() {             // ... and this wave's LDS-DMA halves have landed
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0070);     // vmcnt(0) lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

#ifndef SGLK_PP_PRIO
#define SGLK_PP_PRIO 2
#endif

}  // namespace attn
}  // namespace sglk
