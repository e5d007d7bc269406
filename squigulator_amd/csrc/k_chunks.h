// k_chunks.h -- labelled, normalised signal chunks of a batch (include/sqg_chunks.h): per-read median / MAD, chunk emit, CTC labels
// Part of the device code of the per-read signal path; included through sqg_kernels.h (see there for the overview).
//
//   k_chunk_stats        one workgroup per read: min / max, one exact LDS histogram over [min, max], med2 AND mad4 from that histogram
//                        (deviation counts are histogram bins folded around the median); reads whose codes span more than CHUNK_HIST
//                        bins go on a list, reads longer than the caller's limit are left to the long path
//   k_chunk_stats_wide   the listed reads: a 65536-bin histogram in global memory per workgroup, same selection
//   k_chunk_hist_long, k_chunk_select_long   one long read over many workgroups: global histogram, then the selection by one workgroup
//   k_chunk_consts       the same constants from med2 / mad4 the caller passed in (sqg_batch_chunk_targets with the statistics of an earlier call)
//   k_chunk_index        chunk -> read, chunk -> first sample
//   k_chunk_emit         streaming: 2 B/sample in, the chunk rows out in 16-byte stores (chunk_row8, which k_sites.h's rows go through too)
//   k_chunk_labels       one workgroup per read: one scan of its dwells finds every chunk's event range [e0, e1); then the codes
// Which statistics path a read took shows in no output: all three count the same integers.
// BatchView, defined here, is what these and the kernels of k_targets.h, k_segments.h, k_sites.h, k_events_table.h and k_pileup.h take of the batch.
#pragma once

#define CHUNK_WG 256
#define CHUNK_HIST 4096              // LDS bins of the one-workgroup path (the reference vectors span at most 878 codes per read)
#define CHUNK_GBINS 65536            // every int16 code: the global histograms of the generic paths
#define CHUNK_WIDE_SLOTS 32          // workgroups (and global histogram pairs) of k_chunk_stats_wide
#define CHUNK_BIG (1LL << 60)

// What the chunk kernels take for "the read" when it is not the whole stored read (include/sqg_segments.h: the insert of a read with an
// attached prefix; written per read by k_segments, k_segments.h).  Events and bases count from the read's first; samples in generation order
// from the span's first.  32 bytes.
struct ChunkView {
    long long sh_lo, sh_hi;          // the part of the RNA adaptor's level-shift window inside the span, generation order relative to the span (empty: lo >= hi)
    int ev0, nev;                    // the span's events [ev0, ev0 + nev) of chain 0
    int base0;                       // first base of event ev0
    int pad;                         // (to the struct's 8-byte alignment: written, so that the scratch holds no stale bytes)
};

// What every kernel that reads a finished batch takes of it (h_chunks.h: batch_view): the batch's descriptors, bases, dwells and signal,
// the pore table, and the context's settings.  The callers' parameter structs embed it and add what is their own.
#define SEG_NONE 0                   // no SQG_PREFIX: the whole read is insert
#define SEG_DNA 1                    // stall + adaptor + read, stored order = generation order
#define SEG_RNA 2                    // read + poly-A + adaptor, then the stall chain; stored reversed
struct BatchView {
    const ReadDesc* reads;           // [n_reads]
    const uint8_t* bases;
    const float2* model;             // {level_mean, -}
    const uint16_t* dwell;           // the batch's dwells; null: a constant-dwell context, every dwell is const_sps
    const long long* sig_off;        // [n_reads+1]
    const int16_t* sig;              // the batch's signal slab
    int const_sps, k, meth, rna, n_reads;   // rna: the signal is stored reversed
    int kind;                        // SEG_NONE / SEG_DNA / SEG_RNA
    int p0, p1;                      // SEG_DNA: events of the stall, of stall + adaptor.  SEG_RNA: bases of the poly-A, of poly-A + adaptor
    double range, dig;               // the profile's range and digitisation
};

struct ChunkParams {
    BatchView bv;
    const long long* lo;             // [n_reads] every read's span of the slab, [lo, hi): the batch's sig_off and sig_off + 1, or the
    const long long* hi;             //           spans k_segments wrote
    const ChunkView* view;           // [n_reads] the spans' events and bases; null: the whole read (ReadDesc's ev_off, base_off, ne0)
    // the statistics pass (a job of spans alone: h_chunks.h, spans_open / stats_run)
    int hist_max;                    // bins the LDS path may use (CHUNK_HIST; 0: every read takes the wide path)
    long long one_wg_max;            // samples up to which one workgroup takes a read (beyond: the long path, launched per read by the host)
    float2* consts;                  // [n_reads] {median, 1 / (1.4826 * MAD)} as the emit kernel uses them
    int* med2; int* mad4;            // [n_reads] outputs, may be null
    unsigned int* wide_list;         // [0] reads listed, [1 + i] their indices
    unsigned int* ghist;             // [CHUNK_WIDE_SLOTS][2][CHUNK_GBINS]
    // the chunk calls' plan on top of it
    const long long* chunk_off;      // [n_reads+1] first chunk of every read
    long long n_chunks;
    int L, S, W;
    int* chunk_read;                 // [n_chunks] (the caller's array or scratch)
    int* chunk_read_out; long long* chunk_start_out;   // outputs, may be null
};

// exclusive scan of one value per thread over the workgroup (CHUNK_WG threads); sh: 8 words of LDS; *total <- the sum
__device__ static inline unsigned long long chunk_scan_excl(unsigned long long v, unsigned long long* sh, unsigned long long* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CHUNK_WG / 64; w++) { const unsigned long long s = sh[w]; if (w < wv) before += s; all += s; }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// the bins that hold the elements of rank r1 and r2 (0-based, r1 <= r2 < total) of a histogram of nb bins -> res[0], res[1] (LDS)
template <class Load>
__device__ static inline void chunk_select2(Load load, int nb, unsigned long long r1, unsigned long long r2, unsigned long long* sh, int* res) {
    const int per = (nb + CHUNK_WG - 1) / CHUNK_WG;
    const int lo = min((int)threadIdx.x * per, nb), hi = min(lo + per, nb);
    unsigned long long s = 0, total;
    for (int i = lo; i < hi; i++) s += load(i);
    unsigned long long cum = chunk_scan_excl(s, sh, &total);
    for (int i = lo; i < hi; i++) {
        const unsigned long long cnt = load(i);
        if (r1 - cum < cnt) res[0] = i;                     // (unsigned: false when r1 < cum)
        if (r2 - cum < cnt) res[1] = i;
        cum += cnt;
    }
    __syncthreads();
}

// f(sample) for every sample of p[0, n), the threads of the workgroup `part` of `parts` sharing them; 16-byte loads where p allows
template <class F>
__device__ static inline void chunk_for_samples(const int16_t* p, long long n, long long part, long long parts, F f) {
    long long head = (long long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 1);
    if (head > n) head = n;
    const long long t = part * CHUNK_WG + threadIdx.x, nt = parts * CHUNK_WG;
    for (long long i = t; i < head; i += nt) f((int)p[i]);
    const long long nv = (n - head) >> 3;
    const uint4* q = reinterpret_cast<const uint4*>(p + head);
    for (long long i = t; i < nv; i += nt) {
        const uint4 w = q[i];
        f((int)(int16_t)(w.x & 0xffffu)); f((int)(int16_t)(w.x >> 16)); f((int)(int16_t)(w.y & 0xffffu)); f((int)(int16_t)(w.y >> 16));
        f((int)(int16_t)(w.z & 0xffffu)); f((int)(int16_t)(w.z >> 16)); f((int)(int16_t)(w.w & 0xffffu)); f((int)(int16_t)(w.w >> 16));
    }
    for (long long i = head + (nv << 3) + t; i < n; i += nt) f((int)p[i]);
}

__device__ static inline void chunk_write_stats(const ChunkParams& P, int r, int med2, int mad4) {
    if (P.med2) P.med2[r] = med2;
    if (P.mad4) P.mad4[r] = mad4;
    const double madp = mad4 > 0 ? (double)mad4 / 4.0 : 1.0;
    P.consts[r] = make_float2((float)((double)med2 / 2.0), (float)(1.0 / (1.4826 * madp)));
}

__global__ __launch_bounds__(CHUNK_WG) void k_chunk_stats(ChunkParams P) {
    __shared__ unsigned int h1[CHUNK_HIST], h2[CHUNK_HIST + 1];
    __shared__ unsigned long long sh[8];
    __shared__ int res[2], mm[2 * (CHUNK_WG / 64)];
    const int r = blockIdx.x, t = threadIdx.x;
    const long long o = P.lo[r], n = P.hi[r] - o;
    if (n <= 0) { if (t == 0) chunk_write_stats(P, r, 0, 0); return; }
    if (n > P.one_wg_max) return;                           // the long path's
    const int16_t* p = P.bv.sig + o;
    int mn = 32767, mx = -32768;
    chunk_for_samples(p, n, 0, 1, [&](int v) { mn = min(mn, v); mx = max(mx, v); });
#pragma unroll
    for (int d = 32; d; d >>= 1) { mn = min(mn, __shfl_xor(mn, d, 64)); mx = max(mx, __shfl_xor(mx, d, 64)); }
    if ((t & 63) == 0) { mm[2 * (t >> 6)] = mn; mm[2 * (t >> 6) + 1] = mx; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < CHUNK_WG / 64; w++) { mn = min(mn, mm[2 * w]); mx = max(mx, mm[2 * w + 1]); }
    const int span = mx - mn + 1;
    if (span > P.hist_max) {                                // too wide for LDS: k_chunk_stats_wide
        if (t == 0) { const unsigned int at = atomicAdd(&P.wide_list[0], 1u); P.wide_list[1 + at] = (unsigned int)r; }
        return;
    }
    for (int i = t; i <= span; i += CHUNK_WG) { if (i < span) h1[i] = 0; h2[i] = 0; }
    __syncthreads();
    chunk_for_samples(p, n, 0, 1, [&](int v) { atomicAdd(&h1[v - mn], 1u); });
    __syncthreads();
    const unsigned long long r1 = (unsigned long long)((n - 1) / 2), r2 = (unsigned long long)(n / 2);
    chunk_select2([&](int i) { return (unsigned long long)h1[i]; }, span, r1, r2, sh, res);
    const int med2 = (mn + res[0]) + (mn + res[1]), par = med2 & 1;
    // |2v - med2| has med2's parity for every v: bin (dev - par) / 2 < span
    for (int i = t; i < span; i += CHUNK_WG) {
        const unsigned int cnt = h1[i];
        if (cnt) atomicAdd(&h2[(abs(2 * (mn + i) - med2) - par) >> 1], cnt);
    }
    __syncthreads();
    chunk_select2([&](int i) { return (unsigned long long)h2[i]; }, span, r1, r2, sh, res);
    if (t == 0) chunk_write_stats(P, r, med2, (2 * res[0] + par) + (2 * res[1] + par));
}

// med2 and mad4 of n samples from their complete histogram H over all int16 codes (global memory; H2: as many zeroed words); one workgroup
__device__ static inline void chunk_select_global(unsigned int* H, unsigned int* H2, long long n, unsigned long long* sh, int* res, int* med2_out, int* mad4_out) {
    const unsigned long long r1 = (unsigned long long)((n - 1) / 2), r2 = (unsigned long long)(n / 2);
    auto ld = [](unsigned int* a) { return [a](int i) { return (unsigned long long)__hip_atomic_load(&a[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }; };
    chunk_select2(ld(H), CHUNK_GBINS, r1, r2, sh, res);
    const int med2 = (res[0] - 32768) + (res[1] - 32768), par = med2 & 1;
    __syncthreads();
    for (int i = threadIdx.x; i < CHUNK_GBINS; i += CHUNK_WG) {
        const unsigned int cnt = __hip_atomic_load(&H[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cnt) atomicAdd(&H2[(abs(2 * (i - 32768) - med2) - par) >> 1], cnt);      // dev <= 2 * 65535: bin < CHUNK_GBINS
    }
    __threadfence();
    __syncthreads();
    chunk_select2(ld(H2), CHUNK_GBINS, r1, r2, sh, res);
    *med2_out = med2; *mad4_out = (2 * res[0] + par) + (2 * res[1] + par);
}

__global__ __launch_bounds__(CHUNK_WG) void k_chunk_stats_wide(ChunkParams P) {
    __shared__ unsigned long long sh[8];
    __shared__ int res[2];
    unsigned int* H = P.ghist + (size_t)blockIdx.x * 2 * CHUNK_GBINS;
    unsigned int* H2 = H + CHUNK_GBINS;
    const unsigned int count = P.wide_list[0];
    for (unsigned int at = blockIdx.x; at < count; at += gridDim.x) {
        const int r = (int)P.wide_list[1 + at];
        const long long o = P.lo[r], n = P.hi[r] - o;
        for (int i = threadIdx.x; i < 2 * CHUNK_GBINS; i += CHUNK_WG) __hip_atomic_store(&H[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        __syncthreads();
        chunk_for_samples(P.bv.sig + o, n, 0, 1, [&](int v) { atomicAdd(&H[v + 32768], 1u); });
        __threadfence();
        __syncthreads();
        int med2, mad4;
        chunk_select_global(H, H2, n, sh, res, &med2, &mad4);
        if (threadIdx.x == 0) chunk_write_stats(P, r, med2, mad4);
        __syncthreads();
    }
}

// the long path, read r: H (zeroed by the host) <- the histogram, the workgroups sharing the samples
__global__ __launch_bounds__(CHUNK_WG) void k_chunk_hist_long(ChunkParams P, int r) {
    const long long o = P.lo[r], n = P.hi[r] - o;
    unsigned int* H = P.ghist;
    chunk_for_samples(P.bv.sig + o, n, blockIdx.x, gridDim.x, [&](int v) { atomicAdd(&H[v + 32768], 1u); });
}
__global__ __launch_bounds__(CHUNK_WG) void k_chunk_select_long(ChunkParams P, int r) {
    __shared__ unsigned long long sh[8];
    __shared__ int res[2];
    int med2, mad4;
    chunk_select_global(P.ghist, P.ghist + CHUNK_GBINS, P.hi[r] - P.lo[r], sh, res, &med2, &mad4);
    if (threadIdx.x == 0) chunk_write_stats(P, r, med2, mad4);
}

__global__ __launch_bounds__(CHUNK_WG) void k_chunk_consts(ChunkParams P, const int* __restrict__ med2, const int* __restrict__ mad4) {
    const int r = blockIdx.x * CHUNK_WG + threadIdx.x;
    if (r < P.bv.n_reads) chunk_write_stats(P, r, med2[r], mad4[r]);              // (P.med2 / P.mad4 are null: only the constants are written)
}

__global__ __launch_bounds__(CHUNK_WG) void k_chunk_index(ChunkParams P) {
    const int r = blockIdx.x;
    const long long c0 = P.chunk_off[r], nc = P.chunk_off[r + 1] - c0;
    for (long long j = threadIdx.x; j < nc; j += CHUNK_WG) {
        P.chunk_read[c0 + j] = r;
        if (P.chunk_read_out) P.chunk_read_out[c0 + j] = r;
        if (P.chunk_start_out) P.chunk_start_out[c0 + j] = j * P.S;
    }
}

__device__ static inline unsigned int chunk_f16_bits(float x) {
    // x must be the ROUNDED fp32 product when it is converted: left to itself the compiler folds the multiplication into the conversion
    // (v_fma_mixlo_f16: one rounding of the exact product), which differs from fp32-then-fp16 where the fp32 value is a tie of the fp16 grid
    asm volatile("" : "+v"(x));
    const _Float16 h = (_Float16)x;                        // v_cvt_f16_f32: round to nearest even, subnormals kept
    return (unsigned int)__builtin_bit_cast(unsigned short, h);
}
// the two normalisations of a code (include/sqg_chunks.h); cs: the read's {median, 1 / (1.4826 MAD)}
__device__ static inline float chunk_norm_medmad(int raw, float2 cs) { return ((float)raw - cs.x) * cs.y; }
__device__ static inline float chunk_norm_pa(int raw, double offset, double range, double dig) { return (float)((((double)raw + offset) * range) / dig); }
// 8 consecutive values of a row to out[at ..] (elements; 16-byte aligned): two 16-byte stores of fp32, or one of fp16 (rounded from the fp32 value)
template <bool F32>
__device__ static inline void chunk_store8(void* out, long long at, const float (&x)[8]) {
    if (F32) {
        float4* o = reinterpret_cast<float4*>(static_cast<float*>(out) + at);
        o[0] = make_float4(x[0], x[1], x[2], x[3]);
        o[1] = make_float4(x[4], x[5], x[6], x[7]);
    } else {
        uint4 v;
        v.x = chunk_f16_bits(x[0]) | (chunk_f16_bits(x[1]) << 16); v.y = chunk_f16_bits(x[2]) | (chunk_f16_bits(x[3]) << 16);
        v.z = chunk_f16_bits(x[4]) | (chunk_f16_bits(x[5]) << 16); v.w = chunk_f16_bits(x[6]) | (chunk_f16_bits(x[7]) << 16);
        *reinterpret_cast<uint4*>(static_cast<unsigned short*>(out) + at) = v;
    }
}

// k_chunk_emit's split of a workgroup, for the kernel and for the host that sizes its grid: g8 threads per chunk, cpb chunks at a time
struct ChunkEmitGeom { int g8, cpb; };
__host__ __device__ static inline ChunkEmitGeom chunk_emit_geom(int L) { return {L >> 3, (L >> 3) >= CHUNK_WG ? 1 : CHUNK_WG / (L >> 3)}; }

// 8 consecutive samples from any 2-byte address, normalised (PA: with the read's slow5 offset; else with cs), into a 16-byte-aligned row
// at out[at ..]: the aligned 4-byte words that cover them, shifted when the address is odd -- 20 bytes in, no misaligned wide load is
// issued; 16 or 32 bytes out.  k_chunk_emit and k_site_emit (k_sites.h).
template <bool F32, bool PA>
__device__ static inline void chunk_row8(const BatchView& V, const int16_t* src, float2 cs, double offset, void* out, long long at) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>((uintptr_t)src & ~(uintptr_t)3);
    const bool odd = ((uintptr_t)src & 2) != 0;
    uint32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
    if (odd) {
        const uint32_t a4 = q[4];
        a0 = (a0 >> 16) | (a1 << 16); a1 = (a1 >> 16) | (a2 << 16); a2 = (a2 >> 16) | (a3 << 16); a3 = (a3 >> 16) | (a4 << 16);
    }
    const uint32_t a[4] = {a0, a1, a2, a3};
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int raw = (int)(int16_t)((a[i >> 1] >> (16 * (i & 1))) & 0xffffu);
        x[i] = PA ? chunk_norm_pa(raw, offset, V.range, V.dig) : chunk_norm_medmad(raw, cs);
    }
    chunk_store8<F32>(out, at, x);
}

// A workgroup takes 256 / (L / 8) chunks at a time (one for L >= 2048); a thread 8 consecutive samples (chunk_row8).  PA takes the
// reads' slow5 offsets from the batch's descriptors.
template <bool F32, bool PA>
__global__ __launch_bounds__(CHUNK_WG) void k_chunk_emit(ChunkParams P, void* __restrict__ out) {
    const auto [g8, cpb] = chunk_emit_geom(P.L);
    const int sub = (int)threadIdx.x / g8, w0 = (int)threadIdx.x - sub * g8;
    if (sub >= cpb) return;
    for (long long c = (long long)blockIdx.x * cpb + sub; c < P.n_chunks; c += (long long)gridDim.x * cpb) {
        const int r = P.chunk_read[c];
        const long long j = c - P.chunk_off[r];
        const int16_t* src0 = P.bv.sig + P.lo[r] + j * P.S;
        const float2 cs = P.consts[r];
        double offset = 0.0;
        if (PA) offset = P.bv.reads[r].offset;
        for (int w = w0; w < g8; w += CHUNK_WG) chunk_row8<F32, PA>(P.bv, src0 + (long long)w * 8, cs, offset, out, c * (long long)P.L + (long long)w * 8);
    }
}

// Every chunk boundary g of the read with lo < g <= hi gets event index `value`: the chunk's e0 (which = 0: g is the chunk's first
// generation-order sample) or e1 (which = 1: one past its last).  DNA: g = jS + which L; RNA: g = n - L + which L - jS.  All boundaries lie
// in [0, n], so the interval is cut to that first and the divisions below see small non-negative numbers: 32-bit ones when the read allows
// (64-bit division is a hundred instructions, and every event comes through here four times).
struct ChunkGeom { long long n, nc, c0; int L, S, rna; bool small; };   // small: n < 2^31, the divisions fit 32 bits
__device__ static inline long long chunk_div(long long a, int S, bool small) {   // a >= 0
    return small ? (long long)((uint32_t)a / (uint32_t)S) : a / S;
}
__device__ static inline void chunk_mark(const ChunkGeom& G, int2* ev, long long lo, long long hi, int value) {
    lo = max(lo, -1LL); hi = min(hi, G.n);
    if (hi <= lo) return;
    const bool small = G.small;
#pragma unroll
    for (int which = 0; which < 2; which++) {
        // multiples jS in (a_lo, a_hi]
        long long a_lo, a_hi;
        if (!G.rna) { const long long sh = which ? G.L : 0; a_lo = lo - sh; a_hi = hi - sh; }
        else { const long long A = G.n - (which ? 0 : G.L); a_lo = A - hi - 1; a_hi = A - lo - 1; }
        if (a_hi < 0) continue;
        const long long jlo = a_lo < 0 ? 0 : chunk_div(a_lo, G.S, small) + 1;
        const long long jhi = min(chunk_div(a_hi, G.S, small), G.nc - 1);
        for (long long j = jlo; j <= jhi; j++) { if (which) ev[G.c0 + j].y = value; else ev[G.c0 + j].x = value; }
    }
}

__device__ static inline uint32_t chunk_label_code(uint8_t b, int meth) { return (meth && b == 'M') ? 5u : base_code(b) + 1u; }

// the events and bases the chunks of read r are cut from: the whole of chain 0, or the view's part of it
struct ChunkOrigin { long long ev_off, base_off; int ne; };
__device__ static inline ChunkOrigin chunk_origin(const ChunkParams& P, const ReadDesc& rd, int r) {
    if (!P.view) return {rd.ev_off, rd.base_off, rd.ne0};
    const ChunkView v = P.view[r];
    return {rd.ev_off + v.ev0, rd.base_off + v.base0, v.nev};
}

// E[e], the first sample of event e relative to its read, is the exclusive prefix sum of the read's dwells.  f(e, E[e], dwell[e]) for every
// event of the origin og (e and E count from its first event), the whole workgroup calling: 4 consecutive events per thread, tiles of 4 * CHUNK_WG events, the sum carried from tile
// to tile.  dwell == nullptr: a constant-dwell context, every dwell is const_sps.  sh: the 8 words of chunk_scan_excl.
// The tile form, for a caller with workgroup-wide work of its own per tile (k_sites.h ranks its sites there): g(e0, E[e0], d) once per
// thread and tile, every thread calling -- its 4 events e0 .. e0 + 3 and their dwells, 0 for those behind the origin's last.
template <class G>
__device__ static inline void chunk_for_event_tiles(const ChunkOrigin& og, const uint16_t* dwell, int const_sps, unsigned long long* sh, G g) {
    const int ne = og.ne, t = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < ne; base += 4 * CHUNK_WG) {
        const int e0 = base + 4 * t;
        int d[4];
#pragma unroll
        for (int q = 0; q < 4; q++) d[q] = e0 + q < ne ? (dwell ? (int)dwell[og.ev_off + e0 + q] : const_sps) : 0;
        unsigned long long total;
        const unsigned long long E = carry + chunk_scan_excl((unsigned long long)(d[0] + d[1] + d[2] + d[3]), sh, &total);
        carry += total;
        g(e0, E, d);
    }
}
template <class F>
__device__ static inline void chunk_for_event_starts(const ChunkOrigin& og, const uint16_t* dwell, int const_sps, unsigned long long* sh, F f) {
    const int ne = og.ne;
    chunk_for_event_tiles(og, dwell, const_sps, sh, [&](int e0, unsigned long long E, const int (&d)[4]) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (e0 + q < ne) f(e0 + q, E, d[q]);
            E += (unsigned long long)d[q];
        }
    });
}

// The chunk boundaries in (E[e], E[e] + dwell[e]] belong to event e + 1 (the first event that starts at or behind them), those at or before 0
// to event 0, those behind the last start to n_events.
__global__ __launch_bounds__(CHUNK_WG) void k_chunk_labels(ChunkParams P, int div64, int2* ev, uint8_t* labels, int* label_len) {
    __shared__ unsigned long long sh[8];
    const BatchView& V = P.bv;
    const uint8_t* __restrict__ bases = V.bases;
    const int rna = V.rna, meth = V.meth;
    const int r = blockIdx.x, t = threadIdx.x;
    ChunkGeom G;
    G.c0 = P.chunk_off[r]; G.nc = P.chunk_off[r + 1] - G.c0;
    if (G.nc <= 0) return;
    G.n = P.hi[r] - P.lo[r]; G.L = P.L; G.S = P.S; G.rna = rna;
    G.small = !div64 && G.n < (1LL << 31);                  // div64: the development build's test hook, the 64-bit divisions on every read
    const ChunkOrigin og = chunk_origin(P, V.reads[r], r);
    const int ne = og.ne;
    chunk_for_event_starts(og, V.dwell, V.const_sps, sh, [&, ne](int e, long long E, int d) {
        if (e == 0) chunk_mark(G, ev, -CHUNK_BIG, 0, 0);
        chunk_mark(G, ev, E, e == ne - 1 ? CHUNK_BIG : E + d, e + 1);
    });
    __threadfence();
    __syncthreads();
    const int lane = t & 63;
    const bool pack4 = (P.W & 3) == 0 && ((uintptr_t)labels & 3) == 0;
    for (long long j = t >> 6; j < G.nc; j += CHUNK_WG / 64) {
        const long long c = G.c0 + j;
        const int e0 = min(max(__hip_atomic_load(&ev[c].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0), ne);
        const int e1 = min(max(__hip_atomic_load(&ev[c].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), e0), ne);   // (every index below stays inside the read)
        const int len = e1 - e0;
        if (label_len && lane == 0) label_len[c] = len;
        if (!labels) continue;
        uint8_t* row = labels + c * (long long)P.W;
        for (int x = 4 * lane; x < P.W; x += 256) {
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = x + q;
                const uint32_t code = i < len ? chunk_label_code(bases[og.base_off + (rna ? e1 - 1 - i : e0 + i)], meth) : 0u;
                v |= code << (8 * q);
            }
            if (pack4) *reinterpret_cast<uint32_t*>(row + x) = v;
            else for (int q = 0; q < 4 && x + q < P.W; q++) row[x + q] = (uint8_t)(v >> (8 * q));
        }
    }
}
