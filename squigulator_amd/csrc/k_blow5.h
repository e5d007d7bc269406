// k_blow5.h -- BLOW5 records framed on the device: slow5_rec_to_mem's layout around the svb-zd bytes, inside a zlib stream of STORED blocks
// Part of the device code of the per-read signal path; included through sqg_kernels.h (see there for the overview).
//
// The reference compresses a record inside the worker (src/sim.c:607 -> slow5lib/src/slow5.c:3815-4075 -> slow5_press.c:794: deflate,
// 28 MB/s per host thread): end to end that is what bounds a host that writes BLOW5.  A zlib stream need not compress: RFC 1951
// "stored" blocks (BTYPE 00) carry the bytes as they are, and any inflate -- slow5lib's included -- reads them.  So the record
//   u64 compressed size | 78 01 | { 00/01 | LEN u16 | ~LEN u16 | <= 65535 bytes }* | adler32 (big endian)
// is written here, per read, straight from the device's svb-zd encoding (k_svb.h): the file holds the same records as the reference's
// (field for field, sample for sample: tests read it back through the reference's own slow5lib) in other bytes, 1.3 instead of 0.97
// per sample, and the host's part is one copy and one write.  The raw record (slow5.c:3928-4072; src/gensig.c:171-223):
//   u16 len(read_id) | read_id | u32 read_group | f64 digitisation | f64 offset | f64 range | f64 sampling_rate |
//   u64 bytes of the compressed signal | those bytes | u64 1 | "0" | f64 median_before | i32 read_number | u8 start_mux |
//   u64 start_time [| u8 end_reason]
// SQG_BLOW5_HUFFMAN (k_blow5_huff_size, k_blow5_huff_encode below): the same raw record in
//   u64 compressed size | 78 01 | block A | block B | adler32 (big endian)
// two dynamic-Huffman blocks (BTYPE 10, literals only, HLIT 0, HDIST 1): A codes raw bytes [0, H + min(S, 4 + ceil(count / 4))) -- the
// head up to the svb-zd byte count (H = 2 + idlen + 4 + 32 + 8 bytes), the encoding's u32 count and its key bytes --, B (final) the data
// bytes and the trailer.  Codes of at most 15 bits (code-length code: 7) by the construction kh_huff.h states, the host encoder's
// (h_blow5.h) source text: the device writes the host's bytes.
#pragma once

#define B5_ID_MAX 4096                    // read ids longer than this: the host-zlib mode (the reference's ids are ~40-80 bytes)
#define B5_BLOCK 65535u                   // bytes per stored block
#define B5_ADLER 65521u

struct Blow5Params {
    const uint8_t* svb;                   // the batch's svb-zd encodings (k_svb_encode) ...
    const long long* svb_off;             // [n+1] ... and their offsets
    const long long* sig_off;             // [n+1] samples before each read of the batch (start_time)
    const uint8_t* ids;                   // read ids, back to back
    const long long* id_off;              // [n+1]
    const double* offset;                 // [n]
    const double* median;                 // [n]
    const long long* rec_off;             // [n+1] where each record goes in `out`
    uint8_t* out;
    double digitisation, range, sample_rate;
    long long read_number0;               // read_number of the batch's first read
    unsigned long long start_time0;       // samples written before this batch
    int ont;                              // the end_reason field (--ont-friendly)
    int n;
};

// bytes of a record whose raw form has R bytes (host and device)
__host__ __device__ static inline unsigned long long b5_stored_size(unsigned long long R) {
    const unsigned long long nblk = R ? (R + B5_BLOCK - 1) / B5_BLOCK : 1;
    return 8 + 2 + 5 * nblk + R + 4;
}

// grid: reads, 256 threads
__global__ __launch_bounds__(256) void k_blow5_frame(const Blow5Params P) {
    __shared__ uint8_t hdr[2 + B5_ID_MAX + 4 + 32 + 8];
    __shared__ uint8_t trl[32];
    __shared__ unsigned long long red_a[4], red_b[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i >= P.n) return;
    const unsigned long long idl = (unsigned long long)(P.id_off[i + 1] - P.id_off[i]);
    const unsigned long long S = (unsigned long long)(P.svb_off[i + 1] - P.svb_off[i]);
    const unsigned long long hl = 2 + idl + 4 + 32 + 8, tl = 8 + 1 + 8 + 4 + 1 + 8 + (P.ont ? 1 : 0);
    const unsigned long long R = hl + S + tl;
    const unsigned long long nblk = (R + B5_BLOCK - 1) / B5_BLOCK;
    uint8_t* const out = P.out + P.rec_off[i];
    auto put = [&](uint8_t* dst, const void* src, int nb) { const uint8_t* q = (const uint8_t*)src; for (int j = 0; j < nb; j++) dst[j] = q[j]; };
    for (unsigned long long j = tid; j < idl; j += 256) hdr[2 + j] = P.ids[P.id_off[i] + (long long)j];
    if (tid == 0) {
        const uint16_t l16 = (uint16_t)idl; const uint32_t rg = 0;
        put(hdr, &l16, 2);
        uint8_t* h = hdr + 2 + idl;
        put(h, &rg, 4); put(h + 4, &P.digitisation, 8); put(h + 12, &P.offset[i], 8); put(h + 20, &P.range, 8); put(h + 28, &P.sample_rate, 8);
        put(h + 36, &S, 8);
        const unsigned long long one = 1; const uint8_t ch = '0', mux = 0, er = 0;
        const int32_t rn = (int32_t)(P.read_number0 + i);
        const unsigned long long st = P.start_time0 + (unsigned long long)P.sig_off[i];
        put(trl, &one, 8); trl[8] = ch; put(trl + 9, &P.median[i], 8); put(trl + 17, &rn, 4); trl[21] = mux; put(trl + 22, &st, 8);
        if (P.ont) trl[30] = er;
        const unsigned long long csize = 2 + 5 * nblk + R + 4;
        put(out, &csize, 8);
        out[8] = 0x78; out[9] = 0x01;                              // CMF: deflate, 32 KiB window; FLG: no dictionary, level 0, check bits
    }
    __syncthreads();
    // the block headers
    for (unsigned long long bk = tid; bk < nblk; bk += 256) {
        const unsigned long long r0 = bk * B5_BLOCK;
        const uint32_t len = (uint32_t)((R - r0 < B5_BLOCK) ? R - r0 : B5_BLOCK);
        uint8_t* q = out + 10 + bk * (B5_BLOCK + 5);
        q[0] = bk + 1 == nblk ? 1 : 0;
        q[1] = (uint8_t)len; q[2] = (uint8_t)(len >> 8); q[3] = (uint8_t)~len; q[4] = (uint8_t)(~len >> 8);
    }
    // the bytes, 16 per thread and step, and their Adler-32 sums: A = 1 + sum d, B = R + sum (R - r) d  (mod 65521)
    const uint8_t* const svb = P.svb + P.svb_off[i];
    unsigned long long sa = 0, sb = 0;
    for (unsigned long long r0 = (unsigned long long)tid * 16; r0 < R; r0 += 256 * 16) {
        const unsigned long long r1 = (r0 + 16 < R) ? r0 + 16 : R;
        uint8_t v[16];
        const bool inner = r0 >= hl && r1 <= hl + S && r1 - r0 == 16;
        if (inner) __builtin_memcpy(v, svb + (r0 - hl), 16);
        else for (unsigned long long r = r0; r < r1; r++) v[r - r0] = r < hl ? hdr[r] : r < hl + S ? svb[r - hl] : trl[r - hl - S];
        const unsigned long long p0 = 10 + 5 * (r0 / B5_BLOCK + 1) + r0;
        if (inner && r0 / B5_BLOCK == (r1 - 1) / B5_BLOCK) __builtin_memcpy(out + p0, v, 16);
        else for (unsigned long long r = r0; r < r1; r++) out[10 + 5 * (r / B5_BLOCK + 1) + r] = v[r - r0];
        unsigned long long a16 = 0, b16 = 0;                        // (16 bytes: a16 <= 4080, b16 <= 16 * 255 * 16)
#pragma unroll
        for (int j = 0; j < 16; j++) { const unsigned long long d = (r0 + j < r1) ? v[j] : 0; a16 += d; b16 += d * (unsigned long long)(16 - j); }
        // sum (R - r) d over the run = (R - r0 - 16) * a16 + b16
        sa += a16;
        sb = (sb + ((R - r0 - 16 + B5_ADLER) % B5_ADLER) * a16 + b16) % B5_ADLER;     // (R - r0 - 16 may be negative by < 16 for the last run: + 65521 first)
    }
    sa %= B5_ADLER;
    for (int o = 32; o > 0; o >>= 1) { sa += __shfl_xor(sa, o); sb += __shfl_xor(sb, o); }
    if ((tid & 63) == 0) { red_a[tid >> 6] = sa; red_b[tid >> 6] = sb; }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long A = (1 + red_a[0] + red_a[1] + red_a[2] + red_a[3]) % B5_ADLER;
        const unsigned long long B = (R % B5_ADLER + red_b[0] + red_b[1] + red_b[2] + red_b[3]) % B5_ADLER;
        const uint32_t ad = (uint32_t)(B << 16 | A);
        uint8_t* q = out + 10 + 5 * nblk + R;
        q[0] = (uint8_t)(ad >> 24); q[1] = (uint8_t)(ad >> 16); q[2] = (uint8_t)(ad >> 8); q[3] = (uint8_t)ad;
    }
}

// ---- SQG_BLOW5_HUFFMAN: the same raw records in two dynamic-Huffman blocks each (format and construction: kh_huff.h) ------------------
// Two passes, one workgroup per read, both reading the svb-zd encodings as k_blow5_frame does:
//   k_blow5_huff_size    byte histograms of block A (head + count + keys) and block B (data + trailer) in LDS -- per-wave copies, and
//                        0x00 (77-97 % of the key bytes) counted in registers, not by LDS atomics on one address --; then the two codes,
//                        one lane each in two waves, by kh_huff.h's b5h_build (the host encoder's source text); the codes go to `tab`,
//                        the record's size to `rec_bytes`.  The host scans the sizes into rec_off (it needs them for the shard split anyway).
//   k_blow5_huff_encode  rounds of 16 raw bytes per thread: code lengths, a workgroup scan of bit offsets, the codes OR-ed into an LDS window
//                        (ds_or), the window's whole words copied out; the Adler-32 as k_blow5_frame computes it.
// (a record is whole bytes at its own offset: no byte of the output is shared with another workgroup.)
#include "kh_huff.h"

#define B5H_ROUND 4096                    // raw bytes per round of the encoder: 16 per thread
#define B5H_WIN 2064                      // words of its window: 4096 * 15 + 2 * 1888 (headers) + 30 (end codes) + 31 (carried) bits, + slack

// the raw record's head (u16 idlen | id | rg | 4 f64 | u64 S) and trailer of read i, into LDS (a __syncthreads() must follow)
__device__ static inline void b5_head_trailer(const Blow5Params& P, int i, int tid, unsigned long long idl, unsigned long long S, uint8_t* hdr, uint8_t* trl) {
    auto put = [&](uint8_t* dst, const void* src, int nb) { const uint8_t* q = (const uint8_t*)src; for (int j = 0; j < nb; j++) dst[j] = q[j]; };
    for (unsigned long long j = tid; j < idl; j += 256) hdr[2 + j] = P.ids[P.id_off[i] + (long long)j];
    if (tid == 0) {
        const uint16_t l16 = (uint16_t)idl; const uint32_t rg = 0;
        put(hdr, &l16, 2);
        uint8_t* h = hdr + 2 + idl;
        put(h, &rg, 4); put(h + 4, &P.digitisation, 8); put(h + 12, &P.offset[i], 8); put(h + 20, &P.range, 8); put(h + 28, &P.sample_rate, 8);
        put(h + 36, &S, 8);
        const unsigned long long one = 1; const uint8_t ch = '0', mux = 0, er = 0;
        const int32_t rn = (int32_t)(P.read_number0 + i);
        const unsigned long long st = P.start_time0 + (unsigned long long)P.sig_off[i];
        put(trl, &one, 8); trl[8] = ch; put(trl + 9, &P.median[i], 8); put(trl + 17, &rn, 4); trl[21] = mux; put(trl + 22, &st, 8);
        if (P.ont) trl[30] = er;
    }
}

// raw bytes [r0, r1) (r1 - r0 <= 16) of the record
__device__ static inline void b5_raw16(const uint8_t* hdr, const uint8_t* svb, const uint8_t* trl, unsigned long long hl, unsigned long long S,
                                       unsigned long long r0, unsigned long long r1, uint8_t v[16]) {
    if (r0 >= hl && r1 <= hl + S && r1 - r0 == 16) __builtin_memcpy(v, svb + (r0 - hl), 16);
    else for (unsigned long long r = r0; r < r1; r++) v[r - r0] = r < hl ? hdr[r] : r < hl + S ? svb[r - hl] : trl[r - hl - S];
}

// where block A ends: the head, the svb-zd count and its key bytes (h_blow5.h's blow5_huff_cut)
__device__ static inline unsigned long long b5_huff_cut(const uint8_t* svb, unsigned long long hl, unsigned long long S) {
    if (S < 4) return hl + S;
    const uint32_t count = (uint32_t)svb[0] | (uint32_t)svb[1] << 8 | (uint32_t)svb[2] << 16 | (uint32_t)svb[3] << 24;
    const unsigned long long keys = 4 + ((unsigned long long)count + 3) / 4;
    return hl + (keys < S ? keys : S);
}

// grid: reads, 256 threads.  tab: [2n] codes (block A, block B of each read); rec_bytes: [n] the records' sizes, size prefix included
__global__ __launch_bounds__(256) void k_blow5_huff_size(const Blow5Params P, B5HuffCode* __restrict__ tab, unsigned long long* __restrict__ rec_bytes, int maxbits) {
    __shared__ uint8_t hdr[2 + B5_ID_MAX + 4 + 32 + 8];
    __shared__ uint8_t trl[32];
    __shared__ uint32_t hist[2][4][256];                 // [block][wave][byte]
    __shared__ uint32_t freq[2][B5H_SYMS];
    __shared__ uint16_t sorted[2][B5H_SYMS];
    __shared__ int used[2];
    __shared__ B5HuffWork wk[2];
    __shared__ unsigned long long bits[2];
    const int i = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (i >= P.n) return;
    const unsigned long long idl = (unsigned long long)(P.id_off[i + 1] - P.id_off[i]);
    const unsigned long long S = (unsigned long long)(P.svb_off[i + 1] - P.svb_off[i]);
    const unsigned long long hl = 2 + idl + 4 + 32 + 8, tl = 8 + 1 + 8 + 4 + 1 + 8 + (P.ont ? 1 : 0);
    const unsigned long long R = hl + S + tl;
    const uint8_t* const svb = P.svb + P.svb_off[i];
    const unsigned long long cut = b5_huff_cut(svb, hl, S);
    b5_head_trailer(P, i, tid, idl, S, hdr, trl);
    for (int j = tid; j < 2 * 4 * 256; j += 256) (&hist[0][0][0])[j] = 0;
    if (tid < 2) used[tid] = 0;
    __syncthreads();
    uint32_t z0 = 0, z1 = 0;                              // the zero bytes of each block: counted here, not by atomics on one LDS word
    for (unsigned long long r0 = (unsigned long long)tid * 16; r0 < R; r0 += 256 * 16) {
        const unsigned long long r1 = (r0 + 16 < R) ? r0 + 16 : R;
        uint8_t v[16];
        b5_raw16(hdr, svb, trl, hl, S, r0, r1, v);
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (r0 + j >= r1) break;
            const int blk = r0 + j >= cut;
            if (v[j] == 0) { if (blk) z1++; else z0++; }
            else atomicAdd(&hist[blk][wave][v[j]], 1u);
        }
    }
    for (int o = 32; o > 0; o >>= 1) { z0 += __shfl_xor(z0, o); z1 += __shfl_xor(z1, o); }
    if (lane == 0) { hist[0][wave][0] = z0; hist[1][wave][0] = z1; }   // (no atomic ever touches byte 0)
    __syncthreads();
    for (int j = tid; j < 2 * B5H_SYMS; j += 256) {
        const int blk = j / B5H_SYMS, s = j % B5H_SYMS;
        freq[blk][s] = s == 256 ? 1u : hist[blk][0][s] + hist[blk][1][s] + hist[blk][2][s] + hist[blk][3][s];
    }
    __syncthreads();
    // step 2 of the construction, a symbol per thread (step 1 leaves a literal alphabet as it is: end of block + at least one byte)
    for (int j = tid; j < 2 * B5H_SYMS; j += 256) {
        const int blk = j / B5H_SYMS, s = j % B5H_SYMS;
        if (freq[blk][s]) { sorted[blk][b5h_rank(freq[blk], B5H_SYMS, s)] = (uint16_t)s; atomicAdd(&used[blk], 1); }
    }
    __syncthreads();
    if (lane == 0 && wave < 2)                            // steps 3-6 and the header: one lane per block, in two waves side by side
        bits[wave] = b5h_build(freq[wave], sorted[wave], used[wave], maxbits, wave, &tab[2 * (size_t)i + wave], &wk[wave]);
    __syncthreads();
    if (tid == 0) rec_bytes[i] = 8 + 2 + (bits[0] + bits[1] + 7) / 8 + 4;
}

// grid: reads, 256 threads.  tab: k_blow5_huff_size's codes; P.rec_off: the scan of its sizes
__global__ __launch_bounds__(256) void k_blow5_huff_encode(const Blow5Params P, const B5HuffCode* __restrict__ tab) {
    __shared__ uint8_t hdr[2 + B5_ID_MAX + 4 + 32 + 8];
    __shared__ uint8_t trl[32];
    __shared__ uint32_t code[2][B5H_SYMS];
    __shared__ uint8_t bh[2][B5H_HDR_MAX];
    __shared__ uint32_t win[B5H_WIN];
    __shared__ unsigned long long wsum[4];
    __shared__ unsigned long long red_a[4], red_b[4];
    const int i = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (i >= P.n) return;
    const unsigned long long idl = (unsigned long long)(P.id_off[i + 1] - P.id_off[i]);
    const unsigned long long S = (unsigned long long)(P.svb_off[i + 1] - P.svb_off[i]);
    const unsigned long long hl = 2 + idl + 4 + 32 + 8, tl = 8 + 1 + 8 + 4 + 1 + 8 + (P.ont ? 1 : 0);
    const unsigned long long R = hl + S + tl;
    const uint8_t* const svb = P.svb + P.svb_off[i];
    const unsigned long long cut = b5_huff_cut(svb, hl, S);
    const B5HuffCode* const t = tab + 2 * (size_t)i;
    b5_head_trailer(P, i, tid, idl, S, hdr, trl);
    for (int j = tid; j < 2 * B5H_SYMS; j += 256) code[j / B5H_SYMS][j % B5H_SYMS] = t[j / B5H_SYMS].code[j % B5H_SYMS];
    for (int j = tid; j < 2 * B5H_HDR_MAX; j += 256) bh[j / B5H_HDR_MAX][j % B5H_HDR_MAX] = t[j / B5H_HDR_MAX].hdr[j % B5H_HDR_MAX];
    for (int j = tid; j < B5H_WIN; j += 256) win[j] = 0;
    const uint32_t hbA = t[0].hdr_bits, hbB = t[1].hdr_bits;
    const unsigned long long nbytes = (hbA + t[0].data_bits + hbB + t[1].data_bits + 7) / 8;   // of the deflate data
    uint8_t* const out = P.out + P.rec_off[i];
    uint8_t* const st = out + 10;
    if (tid == 0) {
        const unsigned long long csize = 2 + nbytes + 4;
        for (int j = 0; j < 8; j++) out[j] = (uint8_t)(csize >> (8 * j));
        out[8] = 0x78; out[9] = 0x01;
    }
    __syncthreads();
    const uint32_t eobA = code[0][256], eobB = code[1][256];
    unsigned long long wbase = 0, rstart = 0;             // bits: the window's first (a multiple of 32), the round's first
    unsigned long long sa = 0, sb = 0;
    for (unsigned long long base = 0; base < R; base += B5H_ROUND) {
        const unsigned long long r0 = base + (unsigned long long)tid * 16, r1 = (r0 + 16 < R) ? r0 + 16 : (r0 < R ? R : r0);
        uint8_t v[16];
        if (r0 < r1) b5_raw16(hdr, svb, trl, hl, S, r0, r1, v);
        // the thread's bits: its bytes' codes, block A's header before byte 0, A's end + B's header before byte `cut`, B's end after the last
        uint32_t nb = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (r0 + j >= r1) break;
            const unsigned long long r = r0 + j;
            if (r == 0) nb += hbA;
            if (r == cut) nb += (eobA >> 16) + hbB;
            nb += code[r >= cut][v[j]] >> 16;
            if (r == R - 1) nb += eobB >> 16;
        }
        uint32_t inc = nb;                                // workgroup scan: inclusive in the wave, then the waves before
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if (lane >= o) inc += y; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned long long before = 0, rtotal = 0;
        for (int w = 0; w < 4; w++) { if (w < wave) before += wsum[w]; rtotal += wsum[w]; }
        // emit: a 64-bit accumulator, whole words OR-ed into the window at the thread's bit position
        uint32_t pp = (uint32_t)(rstart + before + inc - nb - wbase);
        unsigned long long acc = 0;
        int k = 0;
        auto flush = [&](uint32_t wv) {
            const uint32_t idx = pp >> 5, sh = pp & 31;
            if (idx < B5H_WIN) atomicOr(&win[idx], wv << sh);
            if (sh && idx + 1 < B5H_WIN) atomicOr(&win[idx + 1], wv >> (32 - sh));
        };
        auto put = [&](uint32_t c, int n) {
            acc |= (unsigned long long)c << k; k += n;
            if (k >= 32) { flush((uint32_t)acc); acc >>= 32; k -= 32; pp += 32; }
        };
        auto put_hdr = [&](const uint8_t* h, uint32_t hb) { for (uint32_t q = 0; q < hb; q += 8) put(h[q / 8], (int)(hb - q < 8 ? hb - q : 8)); };
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (r0 + j >= r1) break;
            const unsigned long long r = r0 + j;
            if (r == 0) put_hdr(bh[0], hbA);
            if (r == cut) { put(eobA & 0xffffu, (int)(eobA >> 16)); put_hdr(bh[1], hbB); }
            const uint32_t c = code[r >= cut][v[j]];
            put(c & 0xffffu, (int)(c >> 16));
            if (r == R - 1) put(eobB & 0xffffu, (int)(eobB >> 16));
        }
        if (k) flush((uint32_t)acc);
        if (r0 < r1) {                                    // Adler-32: A = 1 + sum d, B = R + sum (R - r) d  (mod 65521), as k_blow5_frame
            unsigned long long a16 = 0, b16 = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) { const unsigned long long d = (r0 + j < r1) ? v[j] : 0; a16 += d; b16 += d * (unsigned long long)(16 - j); }
            sa += a16;
            sb = (sb + ((R - r0 - 16 + B5_ADLER) % B5_ADLER) * a16 + b16) % B5_ADLER;
        }
        __syncthreads();
        rstart += rtotal;
        const unsigned long long full = (rstart - wbase) >> 5;    // the window's whole words: out
        const uint32_t carry = win[full];
        for (unsigned long long q = tid; q < full; q += 256) {
            const uint32_t wv = win[q];
            const unsigned long long o = wbase / 8 + 4 * q;
#pragma unroll
            for (int b = 0; b < 4; b++) if (o + b < nbytes) st[o + b] = (uint8_t)(wv >> (8 * b));
        }
        __syncthreads();
        for (int j = tid; j < B5H_WIN; j += 256) win[j] = j == 0 ? carry : 0u;
        wbase += 32 * full;
        __syncthreads();
    }
    sa %= B5_ADLER;
    for (int o = 32; o > 0; o >>= 1) { sa += __shfl_xor(sa, o); sb += __shfl_xor(sb, o); }
    if (lane == 0) { red_a[wave] = sa; red_b[wave] = sb; }
    __syncthreads();
    if (tid == 0) {
        for (unsigned long long q = wbase / 8; q < nbytes; q++) st[q] = (uint8_t)(win[0] >> (8 * (q - wbase / 8)));   // the last < 32 bits
        const unsigned long long A = (1 + red_a[0] + red_a[1] + red_a[2] + red_a[3]) % B5_ADLER;
        const unsigned long long B = (R % B5_ADLER + red_b[0] + red_b[1] + red_b[2] + red_b[3]) % B5_ADLER;
        const uint32_t ad = (uint32_t)(B << 16 | A);
        uint8_t* q = st + nbytes;
        q[0] = (uint8_t)(ad >> 24); q[1] = (uint8_t)(ad >> 16); q[2] = (uint8_t)(ad >> 8); q[3] = (uint8_t)ad;
    }
}
