// extend_attention_fp8kv: prefill attention (paged prefix + causal extend tokens) over a float8_e4m3fn KV cache with one scale
// per tensor.  The per-wave cores (CorePP, Core), the LDS images and swizzles, HalfDma and the slot barriers are those of
// attention.hip (attention_internal.h); the cache write is the decode operator's (attention_fp8kv.hip).  New here is how a cache
// tile reaches LDS, and where the two scales go.
//
// * conversion once per workgroup: the 8 waves of a workgroup all read the same 64-key tiles, so -- unlike the decode kernel, where
//   every wave converts the operands of its own keys in front of the MFMA -- the fp8 bytes become bf16 (exactly, cvt8) on the way
//   INTO LDS, and the rings hold the bf16 image the matrix side already reads: qk / softmax / pv do not know where a tile came from.
// * two-phase kernel (D = DV = 128; extend_pp_kernel<0, 128>'s groups, slots and 96 KiB rings): a group's 32-row half of a cache
//   tile is 4 KiB = ONE 16-byte load per thread (row = t256 / 8, 16 elements from 16 (t256 % 8)).  Page ids are looked up at the start
//   of a matrix slot, the row loads are issued at the end of that slot (where stage_issue sits),
//   and in the softmax slot after that, in front of its barrier, the 16 bytes are converted and written with two ds_write_b128 to
//   the two swizzled slots the bf16 image gives those elements (Swz<16>::mask for K, vswz for V).  The compiler counts the vmcnt of
//   the plain loads itself; the barrier's lgkmcnt(0) publishes the writes.  Extend tiles keep HalfDma's LDS-DMA.
//   A workgroup whose sequence has no prefix takes a branch with the bf16 kernel's own staging loop (see there).
// * the tile stream is NOT the 64-aligned concatenation of attention.hip: the prefix takes ceil(prefix / 64) tiles of its own (the
//   last one partial: rows past the prefix repeat its last row / are zero and are masked by `limit`, probabilities exactly 0), and
//   the extend tokens start a fresh tile.  No tile holds rows of both kinds, at the price of at most one more tile per workgroup
//   when prefix % 64 != 0; no row outside the request is read.
// * scales, without a rounding the decode operator does not have: a tile is all-cache or all-extend, so k_scale rides in the
//   softmax scale of the cache tiles (sm_scale * k_scale), and v_scale multiplies the fp32 accumulator O once, after the P.V of the
//   last cache tile (the running sum l is untouched; the deferred rescale by alpha commutes with it).
// * generic kernel (64/64): extend_attention_kernel<64, 64, 2, 0, 8>'s structure (TileRegs software pipeline, paired query
//   blocks); a cache chunk is loaded as 8 bytes and widened in registers before TileRegs::store.
#include "attention_internal.h"

namespace sglk {
namespace attn {

struct ExtendFp8Params {
    ExtendParams e;          // k_buf / v_buf: the cache BYTES, kb_s* / vb_s* in bytes
    float k_scale, v_scale;
};

// A cache's KvSource carries a byte pointer and a byte stride.  Cache row of key position p (< n_paged), branch-free
// (kv_row_paged); an int64 table contributes its low words (cache rows < 2^31, as in the decode kernel)
SGLK_DEV int cache_tok(const KvSource& s, int p) {
    return s.page_is64 ? (int)reinterpret_cast<const int64_t*>(s.page)[p] : reinterpret_cast<const int*>(s.page)[p];
}
SGLK_DEV const unsigned char* cache_row(const KvSource& s, int tok) {
    return reinterpret_cast<const unsigned char*>(s.buf) + (int64_t)tok * s.buf_stride_tok;
}

// A group's 32-row half of a 64-key cache tile of 128 columns through registers: 256 threads x 16 bytes.
template <bool VIMG>
struct HalfCvt {
    int tok;
    u32x4 raw;
    // rows past `nkeys` repeat the tile's last row (masked by the caller's limit)
    SGLK_DEV void lookup(const KvSource& src, int p0, int nkeys, int grp, int t256) {
        const int row = grp * 32 + (t256 >> 3);
        tok = cache_tok(src, p0 + (row < nkeys ? row : nkeys - 1));
    }
    SGLK_DEV void load(const KvSource& src, int t256) { raw = *reinterpret_cast<const u32x4*>(cache_row(src, tok) + ((t256 & 7) << 4)); }
    SGLK_DEV void store(unsigned char* lds, int grp, int t256) const {
        const int row = grp * 32 + (t256 >> 3), c = (t256 & 7) * 2;      // bf16 chunks c, c + 1 of the row
        const int m = VIMG ? vswz(row) : (row & Swz<16>::mask);
        unsigned char* r = lds + row * 256;
        *reinterpret_cast<bf16x8*>(r + ((c ^ m) << 4)) = cvt8(raw[0], raw[1]);
        *reinterpret_cast<bf16x8*>(r + (((c + 1) ^ m) << 4)) = cvt8(raw[2], raw[3]);
    }
};

// Sequence geometry shared by the two kernels: npc cache tiles, then the extend tiles of the query block.
struct Stream8 {
    int prefix, q_last, npc, nt;
    SGLK_DEV Stream8(int prefix_, int q_last_) : prefix(prefix_), q_last(q_last_) {
        npc = (prefix + kKeys - 1) / kKeys;
        nt = npc + (q_last + kKeys - 1) / kKeys;
    }
    SGLK_DEV bool cache(int t) const { return t < npc; }
    SGLK_DEV int key_base(int t) const { return t < npc ? t * kKeys : prefix + (t - npc) * kKeys; }   // stream position of a tile's first key
    SGLK_DEV int ext0(int t) const { return (t - npc) * kKeys; }                                       // first extend token of an extend tile
    SGLK_DEV int nkeys(int t) const {
        const int r = t < npc ? prefix - t * kKeys : q_last - (t - npc) * kKeys;
        return r < kKeys ? r : kKeys;
    }
};

__global__ __launch_bounds__(512, 2) void extend_pp_fp8kv_kernel(const ExtendFp8Params pp) {
    const ExtendParams& p = pp.e;
    constexpr int D = 128, DV = 128, QT = 2, QB = 256, WQ = 32;
    constexpr int KB = kKeys * D * 2, VB = kKeys * DV * 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char pp8_lds[];   // K ring [3][KB], V ring [3][VB], bf16
    unsigned char* const kring = pp8_lds;
    unsigned char* const vring = pp8_lds + 3 * KB;

    const int lin = blockIdx.x;
    const int nqblk = p.nqblk;
    int b, h, qblk;
    if (p.order & 2) { h = lin % p.HQ; b = (lin / p.HQ) % p.B; qblk = lin / (p.HQ * p.B); }
    else { qblk = lin % nqblk; b = (lin / nqblk) % p.B; h = lin / (nqblk * p.B); }
    const int ext_len = p.b_seq_len_extend[b];
    const int prefix = (int)p.b_seq_len[b] - ext_len;
    const int ext_start = p.b_start_loc_extend[b];
    const int q0 = (nqblk - 1 - qblk) * QB;      // heaviest query blocks first
    if (q0 >= ext_len) return;
    const int kvh = h / (p.HQ / p.HKV);
    const int kvh_buf = p.HBUF == p.HKV ? kvh : 0;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = wave >> 2;
    const int qslot = ((wave & 3) << 1) | grp;
    CorePP<D, SGLK_PP_AHEAD> core;
    core.init();
    int limit[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int qi = q0 + qslot * WQ + qt * 16 + (lane & 15);
        const bool valid = qi < ext_len;
        core.load_q(qt, valid ? p.q + (int64_t)(ext_start + qi) * p.q_s0 + (int64_t)h * p.q_s1 : nullptr, lane);
        limit[qt] = valid ? prefix + qi + 1 : 0;
    }
    // kc / vc: the caches (bytes);  kx / vx: the sequence's extend rows, position 0 = its first extend token
    KvSource kc{}, vc, kx{}, vx;
    kc.buf = reinterpret_cast<const unsigned short*>(reinterpret_cast<const unsigned char*>(p.k_buf) + (int64_t)kvh_buf * p.kb_s1);
    kc.buf_stride_tok = p.kb_s0;
    kc.page = reinterpret_cast<const unsigned char*>(p.req_to_tokens) + p.b_req_idx[b] * p.rtt_stride * (p.rtt_is64 ? 8 : 4);
    kc.page_is64 = p.rtt_is64; kc.n_paged = prefix;
    vc = kc;
    vc.buf = reinterpret_cast<const unsigned short*>(reinterpret_cast<const unsigned char*>(p.v_buf) + (int64_t)kvh_buf * p.vb_s1);
    vc.buf_stride_tok = p.vb_s0;
    kx.ext = p.k_ext + (int64_t)ext_start * p.ke_s0 + (int64_t)kvh * p.ke_s1; kx.ext_stride_tok = p.ke_s0;
    vx = kx;
    vx.ext = p.v_ext + (int64_t)ext_start * p.ve_s0 + (int64_t)kvh * p.ve_s1; vx.ext_stride_tok = p.ve_s0;

    const Stream8 st(prefix, q0 + QB < ext_len ? q0 + QB : ext_len);
    const int nt = st.nt, npc = st.npc;
    const int wave_q_last = (q0 + qslot * WQ + WQ < ext_len) ? q0 + qslot * WQ + WQ : ext_len;
    const int nt_w = q0 + qslot * WQ < ext_len ? npc + (wave_q_last + kKeys - 1) / kKeys : 0;   // tiles this wave's queries can see
    const float scale_x = p.sm_scale * 1.4426950408889634f, scale_c = scale_x * pp.k_scale;

    const int t256 = threadIdx.x & 255, wv = t256 >> 6;
    HalfDma<D, 1> kd;
    HalfDma<DV, 1, true> vd;
    if (npc == 0) {
        // No cache tile (a prefill without a cached prefix, the most common call): extend_pp_kernel's own staging and loop -- source
        // pointers at the start of the softmax slot, LDS-DMA at the end of the matrix slot -- so that the call costs what it costs on
        // the bf16 operator.  The loop below, which also serves cache tiles, is 6 % slower on such a sequence.
        kd.prep(kx, 0, st.nkeys(0), grp, t256); kd.issue(kring, grp, wv);
        vd.prep(vx, 0, st.nkeys(0), grp, t256); vd.issue(vring, grp, wv);
        if (nt > 1) { kd.prep(kx, kKeys, st.nkeys(1), grp, t256); kd.issue(kring + KB, grp, wv); }
        auto stage_prep = [&](int t) __attribute__((always_inline)) {
            if (t + 2 < nt) kd.prep(kx, (t + 2) * kKeys, st.nkeys(t + 2), grp, t256);
            if (t + 1 < nt) vd.prep(vx, (t + 1) * kKeys, st.nkeys(t + 1), grp, t256);
        };
        auto stage_issue = [&](int t) __attribute__((always_inline)) {
            if (t + 2 < nt) kd.issue(kring + ((t + 2) % 3) * KB, grp, wv);
            if (t + 1 < nt) vd.issue(vring + ((t + 1) % 3) * VB, grp, wv);
        };
        stage_prep(0);
        slot_barrier_v();
        if (grp == 1) slot_barrier_m();
        if (nt_w > 0) core.qk(kring, lane);
        stage_issue(0);
        slot_barrier_m();
        for (int t = 0; t < nt; ++t) {
            stage_prep(t + 1);
            if (t < nt_w) core.softmax(t * kKeys, limit, scale_x, p.logit_cap, lane);
            slot_barrier_v();
            __builtin_amdgcn_s_setprio(SGLK_PP_PRIO);
            if (t < nt_w) core.pv(vring + (t % 3) * VB, lane);
            if (t + 1 < nt_w) core.qk(kring + ((t + 1) % 3) * KB, lane);
            __builtin_amdgcn_s_setprio(0);
            stage_issue(t + 1);
            slot_barrier_m();
        }
    } else {
        HalfCvt<false> kq;
        HalfCvt<true> vq;
        // ---- prologue: K_0, K_1, V_0, each group its halves; lookups, row loads and conversions of the three back to back ----
        {
            HalfCvt<false> kq1;
            if (st.cache(0)) { kq.lookup(kc, 0, st.nkeys(0), grp, t256); vq.lookup(vc, 0, st.nkeys(0), grp, t256); }
            if (nt > 1 && st.cache(1)) kq1.lookup(kc, kKeys, st.nkeys(1), grp, t256);
            if (st.cache(0)) { kq.load(kc, t256); vq.load(vc, t256); }
            else {
                kd.prep(kx, 0, st.nkeys(0), grp, t256); kd.issue(kring, grp, wv);
                vd.prep(vx, 0, st.nkeys(0), grp, t256); vd.issue(vring, grp, wv);
            }
            if (nt > 1) {
                if (st.cache(1)) kq1.load(kc, t256);
                else { kd.prep(kx, st.ext0(1), st.nkeys(1), grp, t256); kd.issue(kring + KB, grp, wv); }
            }
            if (st.cache(0)) { kq.store(kring, grp, t256); vq.store(vring, grp, t256); }
            if (nt > 1 && st.cache(1)) kq1.store(kring + KB, grp, t256);
        }
        // the halves that travel around V_t: K_{t+2}, V_{t+1}.  prep: the page lookups of cache rows, at the start of the matrix slot (not
        // one slot earlier, as the bf16 kernel's: across a softmax slot the registers hold the rows); issue, at the end of that slot: row loads into registers, or -- extend rows need no
        // lookup, their source pointers are arithmetic -- HalfDma's prep and LDS-DMA back to back; store: cache rows only, converted and
        // written at the end of the next softmax slot
        // (the staging addresses are the same for every tile; hoisted out of the tile loop they would occupy a dozen registers beside
        // q, the accumulator and the rows in flight, so each stage starts from an opaque copy of the thread index)
        auto opaque = [](int v) __attribute__((always_inline)) { asm volatile("" : "+v"(v)); return v; };
        auto stage_prep = [&](int t) __attribute__((always_inline)) {
            const int t256 = opaque(threadIdx.x) & 255;
            if (t + 2 < npc) kq.lookup(kc, (t + 2) * kKeys, st.nkeys(t + 2), grp, t256);
            if (t + 1 < npc) vq.lookup(vc, (t + 1) * kKeys, st.nkeys(t + 1), grp, t256);
        };
        auto stage_issue = [&](int t) __attribute__((always_inline)) {
            const int t256 = opaque(threadIdx.x) & 255;
            if (t + 2 < nt) {
                if (st.cache(t + 2)) kq.load(kc, t256);
                else { kd.prep(kx, st.ext0(t + 2), st.nkeys(t + 2), grp, t256); kd.issue(kring + ((t + 2) % 3) * KB, grp, wv); }
            }
            if (t + 1 < nt) {
                if (st.cache(t + 1)) vq.load(vc, t256);
                else { vd.prep(vx, st.ext0(t + 1), st.nkeys(t + 1), grp, t256); vd.issue(vring + ((t + 1) % 3) * VB, grp, wv); }
            }
        };
        auto stage_store = [&](int t) __attribute__((always_inline)) {
            const int t256 = opaque(threadIdx.x) & 255;
            if (t + 2 < npc) kq.store(kring + ((t + 2) % 3) * KB, grp, t256);
            if (t + 1 < npc) vq.store(vring + ((t + 1) % 3) * VB, grp, t256);
        };
        stage_prep(0);
        slot_barrier_v();
        if (grp == 1) slot_barrier_m();             // slot 0: group B idles
        // slot: S_0
        if (nt_w > 0) core.qk(kring, lane);
        stage_issue(0);
        slot_barrier_m();
        for (int t = 0; t < nt; ++t) {
            // ---- V_t ----
            if (t < nt_w) {
                // a cache tile: the keys below the prefix, visible to every valid query (limit > prefix), at the cache's scale
                const bool c = st.cache(t);
                const int top = c ? prefix : 0x7fffffff;
                const int lim[QT] = {limit[0] < top ? limit[0] : top, limit[1] < top ? limit[1] : top};
                core.softmax(st.key_base(t), lim, c ? scale_c : scale_x, p.logit_cap, lane);
            }
            stage_store(t);                         // the cache halves loaded one slot ago: bf16 into the rings
            slot_barrier_v();                       // ... and the LDS-DMA halves issued one slot ago have landed
            // ---- M_t ----
            stage_prep(t + 1);                      // in flight during the slot, consumed at its end
            __builtin_amdgcn_s_setprio(SGLK_PP_PRIO);
            if (t < nt_w) core.pv(vring + (t % 3) * VB, lane);
            if (t + 1 < nt_w) core.qk(kring + ((t + 1) % 3) * KB, lane);
            __builtin_amdgcn_s_setprio(0);
            if (t == npc - 1) {                     // O so far is the cache's: its scale once, in fp32
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                    for (int i = 0; i < DV / 16; ++i) core.o[qt][i] *= pp.v_scale;
            }
            stage_issue(t + 1);                     // behind the slot's last LDS read
            slot_barrier_m();
        }
    }
    if (grp == 0) slot_barrier_m();             // last slot: group A idles
    // ---- normalise and store ----
    const int g4 = (lane >> 4) * 4;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const float lsum = core.column_sum(qt);
        const int qi = q0 + qslot * WQ + qt * 16 + (lane & 15);
        if (qi >= ext_len) continue;
        const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
        unsigned short* orow = p.o + (int64_t)(ext_start + qi) * p.o_s0 + (int64_t)h * p.o_s1;
#pragma unroll
        for (int t = 0; t < DV / 16; ++t) {
            const f32x4 v = core.o[qt][t] * inv;
            uint2 w;
            w.x = pack_bf16x2(v[0], v[1]);
            w.y = pack_bf16x2(v[2], v[3]);
            *reinterpret_cast<uint2*>(orow + t * 16 + g4) = w;
        }
    }
}

// TileRegs whose cache tiles travel as bytes: a chunk of 8 elements is 8 bytes in v[i].x / .y until widen()
template <int WIDTH, int THREADS>
struct TileRegs8 : TileRegs<WIDTH, THREADS> {
    typedef TileRegs<WIDTH, THREADS> Base;
    SGLK_DEV void load_cache(const KvSource& src, int p0, int nkeys) {
        const unsigned char* rp[Base::NCH];
#pragma unroll
        for (int i = 0; i < Base::NCH; ++i) {
            const int c = threadIdx.x + i * THREADS;
            const int row = c / Base::CH, ch = c - row * Base::CH;
            rp[i] = (c < kKeys * Base::CH && row < nkeys) ? cache_row(src, cache_tok(src, p0 + row)) + ch * 8 : nullptr;
        }
#pragma unroll
        for (int i = 0; i < Base::NCH; ++i) {
            this->v[i] = make_uint4(0, 0, 0, 0);
            if (!rp[i]) continue;
            const uint2 w = *reinterpret_cast<const uint2*>(rp[i]);
            this->v[i].x = w.x;
            this->v[i].y = w.y;
        }
    }
    SGLK_DEV void widen() {
#pragma unroll
        for (int i = 0; i < Base::NCH; ++i) this->v[i] = __builtin_bit_cast(uint4, cvt8(this->v[i].x, this->v[i].y));
    }
};

template <int D, int DV>
__global__ __launch_bounds__(512, 2) void extend_fp8kv_kernel(const ExtendFp8Params pp) {
    const ExtendParams& p = pp.e;
    constexpr int QT = 2, NW = 8, QB = NW * QT * 16, WQ = QT * 16;
    constexpr int KB = kKeys * D * 2, VB = kKeys * DV * 2;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * (KB + VB)];   // two {K, V} tile buffers, bf16

    // workgroup-id decomposition and paired query blocks: extend_attention_kernel
    int lin = blockIdx.x;
    {
        const int total = gridDim.x, hi = 2 * p.n_cu < total ? 2 * p.n_cu : total;
        if ((p.order & 1) && lin >= p.n_cu && lin < hi) lin = p.n_cu + hi - 1 - lin;
    }
    const int nqblk = p.nqblk;
    const int nitem = p.pair ? (nqblk + 1) / 2 : nqblk;
    int b, h, qblk0;
    if (p.order & 2) { h = lin % p.HQ; b = (lin / p.HQ) % p.B; qblk0 = lin / (p.HQ * p.B); }
    else { qblk0 = lin % nitem; b = (lin / nitem) % p.B; h = lin / (nitem * p.B); }
    const int ext_len = p.b_seq_len_extend[b];
    const int prefix = (int)p.b_seq_len[b] - ext_len;
    const int ext_start = p.b_start_loc_extend[b];
    const int kvh = h / (p.HQ / p.HKV);
    const int kvh_buf = p.HBUF == p.HKV ? kvh : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    KvSource kc{}, vc, kx{}, vx;
    kc.buf = reinterpret_cast<const unsigned short*>(reinterpret_cast<const unsigned char*>(p.k_buf) + (int64_t)kvh_buf * p.kb_s1);
    kc.buf_stride_tok = p.kb_s0;
    kc.page = reinterpret_cast<const unsigned char*>(p.req_to_tokens) + p.b_req_idx[b] * p.rtt_stride * (p.rtt_is64 ? 8 : 4);
    kc.page_is64 = p.rtt_is64; kc.n_paged = prefix;
    vc = kc;
    vc.buf = reinterpret_cast<const unsigned short*>(reinterpret_cast<const unsigned char*>(p.v_buf) + (int64_t)kvh_buf * p.vb_s1);
    vc.buf_stride_tok = p.vb_s0;
    kx.ext = p.k_ext + (int64_t)ext_start * p.ke_s0 + (int64_t)kvh * p.ke_s1; kx.ext_stride_tok = p.ke_s0;   // n_paged = 0: kv_row() takes ext
    vx = kx;
    vx.ext = p.v_ext + (int64_t)ext_start * p.ve_s0 + (int64_t)kvh * p.ve_s1; vx.ext_stride_tok = p.ve_s0;
    const float scale_x = p.sm_scale * 1.4426950408889634f, scale_c = scale_x * pp.k_scale;

    for (int part = 0; part < (p.pair ? 2 : 1); ++part) {
    const int qblk = part == 0 ? qblk0 : nqblk - 1 - qblk0;
    if (part == 1 && qblk == qblk0) break;
    const int q0 = (nqblk - 1 - qblk) * QB;
    if (q0 >= ext_len) continue;
    Core<D, DV, QT> core;
    core.init();
    int limit[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int qi = q0 + wave * WQ + qt * 16 + (lane & 15);
        const bool valid = qi < ext_len;
        core.load_q(qt, valid ? p.q + (int64_t)(ext_start + qi) * p.q_s0 + (int64_t)h * p.q_s1 : nullptr, lane);
        limit[qt] = valid ? prefix + qi + 1 : 0;
    }
    const Stream8 st(prefix, q0 + QB < ext_len ? q0 + QB : ext_len);
    const int wave_q_last = (q0 + wave * WQ + WQ < ext_len) ? q0 + wave * WQ + WQ : ext_len;
    const int nt_w = q0 + wave * WQ < ext_len ? st.npc + (wave_q_last + kKeys - 1) / kKeys : 0;

    // software pipeline of extend_attention_kernel: tile t+1 travels HBM -> registers while tile t is multiplied out of LDS
    TileRegs8<D, NW * 64> kreg;
    TileRegs8<DV, NW * 64> vreg;
    auto load = [&](int t) {
        if (st.cache(t)) { kreg.load_cache(kc, t * kKeys, st.nkeys(t)); vreg.load_cache(vc, t * kKeys, st.nkeys(t)); }
        else { kreg.load(kx, st.ext0(t), st.nkeys(t)); vreg.load(vx, st.ext0(t), st.nkeys(t)); }
    };
    auto store = [&](int t, unsigned char* buf) {
        if (st.cache(t)) { kreg.widen(); vreg.widen(); }
        kreg.store(buf);
        vreg.store(buf + KB);
    };
    load(0);
    store(0, lds);
    __syncthreads();
    for (int t = 0; t < st.nt; ++t) {
        unsigned char* cur = lds + (t & 1) * (KB + VB);
        unsigned char* nxt = lds + ((t + 1) & 1) * (KB + VB);
        const bool more = t + 1 < st.nt;
        if (more) load(t + 1);
        if (t < nt_w) {
            const bool c = st.cache(t);
            const int top = c ? prefix : 0x7fffffff;
            const int lim[QT] = {limit[0] < top ? limit[0] : top, limit[1] < top ? limit[1] : top};
            core.template tile<false>(cur, cur + KB, st.key_base(t), lim, c ? scale_c : scale_x, p.logit_cap, lane);
        }
        if (t == st.npc - 1) {                  // O so far is the cache's: its scale once, in fp32
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int i = 0; i < DV / 16; ++i) core.o[qt][i] *= pp.v_scale;
        }
        if (more) store(t + 1, nxt);
        __syncthreads();
    }
    const int g4 = (lane >> 4) * 4;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const float lsum = core.column_sum(qt);
        const int qi = q0 + wave * WQ + qt * 16 + (lane & 15);
        if (qi >= ext_len) continue;
        const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
        unsigned short* orow = p.o + (int64_t)(ext_start + qi) * p.o_s0 + (int64_t)h * p.o_s1;
#pragma unroll
        for (int t = 0; t < DV / 16; ++t) {
            const f32x4 v = core.o[qt][t] * inv;
            uint2 w;
            w.x = pack_bf16x2(v[0], v[1]);
            w.y = pack_bf16x2(v[2], v[3]);
            *reinterpret_cast<uint2*>(orow + t * 16 + g4) = w;
        }
    }
    }   // part
}

}  // namespace attn
}  // namespace sglk

using namespace sglk;
using namespace sglk::attn;

extern "C" int sglk_extend_attention_fp8kv(const sglk_extend_attention_fp8kv_args* a, void* stream) {
    const char* const op = "extend_attention_fp8kv";
    SGLK_REQUIRE(a, SGLK_ERR_INVALID, "%s: null args", op);
    SGLK_REQUIRE(a->B >= 0 && a->HQ > 0 && a->HKV > 0 && a->HQ % a->HKV == 0, SGLK_ERR_INVALID, "%s: bad head counts HQ=%d HKV=%d", op,
                 a->HQ, a->HKV);
    SGLK_REQUIRE(a->HBUF == a->HKV || a->HBUF == 1, SGLK_ERR_SHAPE, "%s: buffer heads (%d) must equal HKV (%d) or 1", op, a->HBUF, a->HKV);
    SGLK_REQUIRE(a->k_scale > 0.f && a->k_scale <= 3.0e38f && a->v_scale > 0.f && a->v_scale <= 3.0e38f, SGLK_ERR_INVALID,
                 "%s: k_scale and v_scale must be positive and finite", op);
    SGLK_REQUIRE((a->D == 128 && a->DV == 128) || (a->D == 64 && a->DV == 64), SGLK_ERR_SHAPE,
                 "%s: head dims D=%d DV=%d not built (have 128/128, 64/64)", op, a->D, a->DV);
    SGLK_REQUIRE(!a->out_cache_loc || a->HBUF == a->HKV, SGLK_ERR_SHAPE, "%s: the cache write needs buffers with HKV heads (have %d)", op,
                 a->HBUF);
    SGLK_REQUIRE(a->T >= 0, SGLK_ERR_INVALID, "%s: negative token count", op);
    if (a->B == 0 || a->max_len_extend <= 0) return SGLK_OK;
    SGLK_REQUIRE(a->q && a->k_extend && a->v_extend && a->o && a->k_buffer && a->v_buffer && a->req_to_tokens && a->b_req_idx &&
                     a->b_seq_len && a->b_seq_len_extend && a->b_start_loc_extend, SGLK_ERR_INVALID, "%s: null pointer", op);
    ExtendFp8Params pp{};
    ExtendParams& p = pp.e;
    p.q = (const unsigned short*)a->q; p.k_ext = (const unsigned short*)a->k_extend; p.v_ext = (const unsigned short*)a->v_extend;
    p.k_buf = (const unsigned short*)a->k_buffer; p.v_buf = (const unsigned short*)a->v_buffer; p.o = (unsigned short*)a->o;
    p.q_s0 = a->q_stride[0]; p.q_s1 = a->q_stride[1]; p.ke_s0 = a->k_extend_stride[0]; p.ke_s1 = a->k_extend_stride[1];
    p.ve_s0 = a->v_extend_stride[0]; p.ve_s1 = a->v_extend_stride[1]; p.kb_s0 = a->k_buffer_stride[0]; p.kb_s1 = a->k_buffer_stride[1];
    p.vb_s0 = a->v_buffer_stride[0]; p.vb_s1 = a->v_buffer_stride[1]; p.o_s0 = a->o_stride[0]; p.o_s1 = a->o_stride[1];
    p.req_to_tokens = a->req_to_tokens; p.rtt_stride = a->req_to_tokens_stride; p.rtt_is64 = a->req_to_tokens_is64;
    p.b_req_idx = a->b_req_idx; p.b_seq_len = a->b_seq_len; p.b_seq_len_extend = a->b_seq_len_extend;
    p.b_start_loc_extend = a->b_start_loc_extend; p.HQ = a->HQ; p.HKV = a->HKV; p.HBUF = a->HBUF;
    p.sm_scale = a->sm_scale; p.logit_cap = a->logit_cap;
    p.d_real = a->D; p.dv_real = a->DV; p.v_aligned = 1;
    pp.k_scale = a->k_scale; pp.v_scale = a->v_scale;
    // 16-byte row accesses
    for (int64_t st : {p.q_s0, p.q_s1, p.ke_s0, p.ke_s1, p.ve_s0, p.ve_s1})
        SGLK_REQUIRE(st % 8 == 0, SGLK_ERR_SHAPE, "%s: q/k/v strides must be multiples of 8 elements", op);
    SGLK_REQUIRE(((uintptr_t)a->q % 16) == 0 && ((uintptr_t)a->k_extend % 16) == 0 && ((uintptr_t)a->v_extend % 16) == 0, SGLK_ERR_SHAPE,
                 "%s: q / k_extend / v_extend must be 16-byte aligned", op);
    SGLK_REQUIRE(p.o_s0 % 4 == 0 && p.o_s1 % 4 == 0 && ((uintptr_t)a->o % 8) == 0, SGLK_ERR_SHAPE,
                 "%s: o strides must be multiples of 4 elements", op);
    for (int64_t st : {p.kb_s0, p.kb_s1, p.vb_s0, p.vb_s1})
        SGLK_REQUIRE(st % 16 == 0, SGLK_ERR_SHAPE, "%s: cache strides must be multiples of 16 bytes", op);
    SGLK_REQUIRE(((uintptr_t)a->k_buffer % 16) == 0 && ((uintptr_t)a->v_buffer % 16) == 0, SGLK_ERR_SHAPE,
                 "%s: cache base pointers must be 16-byte aligned", op);
    hipStream_t s = (hipStream_t)stream;
    p.B = a->B; p.n_cu = attn_cus(); p.order = attn_order(2);
    const bool pp_form = a->D == 128;
    constexpr int kPpLds = 3 * kKeys * (128 + 128) * 2;
    int64_t wgs;
    if (pp_form) {
        p.nqblk = (int)ceil_div(a->max_len_extend, 256);
        p.pair = 0;
        wgs = (int64_t)p.nqblk * a->B * a->HQ;
    } else {
        p.nqblk = (int)ceil_div(a->max_len_extend, 256);
        p.pair = pair_blocks(p.nqblk, (int64_t)p.nqblk * a->B * a->HQ, p.n_cu, 1);
        wgs = (int64_t)(p.pair ? (p.nqblk + 1) / 2 : p.nqblk) * a->B * a->HQ;
    }
    SGLK_REQUIRE(wgs < (1ll << 31), SGLK_ERR_SHAPE, "%s: too many workgroups", op);
    if (pp_form) SGLK_ENSURE_DYN_LDS(extend_pp_fp8kv_kernel, kPpLds, "extend_attention_fp8kv");
    // every check has passed.  The write goes first on the stream: the attention reads the prefix only, never these rows
    if (a->out_cache_loc) {
        const int rc = launch_kv_cache_write_fp8(a->k_buffer, a->k_buffer_stride, a->v_buffer, a->v_buffer_stride, a->k_extend,
                                                 a->k_extend_stride, a->v_extend, a->v_extend_stride, a->out_cache_loc,
                                                 a->out_cache_loc_is64, a->T, a->HKV, a->D, a->DV, 0, a->k_scale, a->v_scale, s);
        if (rc != SGLK_OK) return rc;
    }
    if (pp_form) hipLaunchKernelGGL(extend_pp_fp8kv_kernel, dim3((unsigned)wgs), dim3(512), kPpLds, s, pp);
    else hipLaunchKernelGGL((extend_fp8kv_kernel<64, 64>), dim3((unsigned)wgs), dim3(512), 0, s, pp);
    SGLK_CHECK_LAUNCH(op);
    return SGLK_OK;
}
