// kh_huff.h -- the dynamic-Huffman deflate blocks of the BLOW5 writer's SQG_BLOW5_HUFFMAN mode: code construction and block header
// One source text for both sides: included by k_blow5.h (hipcc: the functions are __host__ __device__; k_blow5_huff_size runs
// b5h_build in one lane per block) and by h_blow5.h (the host encoder; g++ builds it as plain C++17 for the CPU backend).
//
// A record's zlib stream is 78 01 | block A | block B | Adler-32, both blocks BTYPE 10 (dynamic Huffman), literals only.  Block A codes
// the raw record's bytes [0, cut) -- the head (u16 idlen | id | rg | 4 f64 | u64 svb bytes), the svb-zd count and the key bytes --,
// block B (BFINAL) the rest: the svb-zd data bytes and the trailer.  cut = H + min(S, 4 + ceil(count / 4)), H = 2 + idlen + 4 + 32 + 8,
// S the svb-zd bytes, count the encoding's own first u32 (the read's samples).  Key bytes and data bytes have different statistics:
// one code each.
//
// Construction of one code (deterministic: the host and the device emit the same bits):
//   1. freq[s]: the block's byte counts, freq[256] = 1 (end of block).  An alphabet with fewer than two used symbols gets frequency 1
//      for its lowest unused symbols until it has two (a literal block never needs it: end of block plus at least one byte).
//   2. the used symbols in ascending (freq, symbol) order (b5h_rank).
//   3. Huffman's tree by the two-queue method: each merge takes the lighter head of the leaf queue and the node queue, the leaf when
//      they weigh the same.
//   4. the leaves' depths, clamped to maxbits; then the Kraft repair: while sum 2^(maxbits - len) > 2^maxbits, one code of length
//      maxbits goes and the longest code shorter than maxbits splits into two one bit longer.
//   5. the lengths dealt out again by count: the count[maxbits] first symbols of the order of step 2 get maxbits, the next
//      count[maxbits - 1] get maxbits - 1, and so on (the least frequent get the longest codes).
//   6. canonical codes, RFC 1951 3.2.2; sent bit-reversed (deflate packs a Huffman code most significant bit first).
// Block header: BFINAL | BTYPE 10 | HLIT 0 (257 literal/length codes) | HDIST 1 (two distance codes of length 1: zlib's literal-only
// convention, which every inflate accepts) | HCLEN | the code-length code's lengths, 3 bits each in RFC order (16 17 18 0 8 7 9 6 10
// 5 11 4 12 3 13 2 14 1 15), trailing zeros dropped, at least 4 | the 257 literal lengths, then the 2 distance lengths, each run-length
// coded on its own:
//   a run of zeros: 18 (11-138 zeros) while >= 11 remain, then 17 (3-10) if >= 3 remain, else single 0s;
//   a run of a length v > 0: v once, then 16 (3-6 repeats) while >= 3 repeats remain, then v for each one left.
// The code-length code is built by steps 1-6 over its 19 symbols with maxbits 7.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define B5H_HD __host__ __device__
#else
#define B5H_HD
#endif

#define B5H_SYMS 257                      // 256 literals + end of block
#define B5H_MAXBITS 15                    // deflate's limit for literal/length codes
#define B5H_CL_MAXBITS 7                  // ... and for the code-length code
#define B5H_HDR_MAX 256                   // bytes of a block header: at most 17 + 19 * 3 + 259 * 7 bits = 236 bytes

struct B5HuffCode {                       // one block's code, ready to emit
    uint32_t code[B5H_SYMS];              // bit-reversed code | length << 16
    uint8_t hdr[B5H_HDR_MAX];             // the block header, LSB first (RFC 1951 bit order)
    uint32_t hdr_bits;
    uint32_t pad_;
    unsigned long long data_bits;         // sum freq[s] * length[s] over the block, end of block included
};

struct B5HuffWork {                       // scratch of one b5h_build
    uint32_t w[2 * B5H_SYMS];             // weights: leaves [0, m), then the merged nodes
    uint16_t up[2 * B5H_SYMS];            // parent of each node, then its depth
    uint16_t rle[2 * B5H_SYMS];           // the run-length coded lengths: symbol | extra << 8
    uint8_t len[B5H_SYMS];                // code lengths by symbol
    uint32_t clf[19];                     // the code-length code: frequencies ...
    uint16_t cls[19];                     //   ... used symbols in order ...
    uint8_t cll[19];                      //   ... lengths
    uint32_t clc[19];                     //   ... and codes (bit-reversed | length << 16)
};

// step 1: returns the number of used symbols
B5H_HD inline int b5h_prepare(uint32_t* freq, int nsym) {
    int m = 0;
    for (int s = 0; s < nsym; s++) m += freq[s] != 0;
    for (int s = 0; s < nsym && m < 2; s++) if (!freq[s]) { freq[s] = 1; m++; }
    return m;
}

// step 2: the place of used symbol s in ascending (freq, symbol) order
B5H_HD inline int b5h_rank(const uint32_t* freq, int nsym, int s) {
    const uint32_t f = freq[s];
    int r = 0;
    for (int t = 0; t < nsym; t++) {
        const uint32_t g = freq[t];
        r += (g != 0) & ((g < f) | ((g == f) & (t < s)));
    }
    return r;
}

B5H_HD inline void b5h_sort(const uint32_t* freq, int nsym, uint16_t* sorted) {
    for (int s = 0; s < nsym; s++) if (freq[s]) sorted[b5h_rank(freq, nsym, s)] = (uint16_t)s;
}

// steps 3-5: len[sorted[0..m)] (other entries untouched); w, up: 2m - 1 entries of scratch
B5H_HD inline void b5h_lengths(const uint32_t* freq, const uint16_t* sorted, int m, int maxbits, uint8_t* len, uint32_t* w, uint16_t* up) {
    for (int j = 0; j < m; j++) w[j] = freq[sorted[j]];
    int li = 0, ni = m;                                   // heads of the leaf queue and of the node queue
    for (int k = m; k < 2 * m - 1; k++) {                 // node k: the merge of the two lightest heads
        uint32_t sum = 0;
        for (int t = 0; t < 2; t++) {
            const int take = (li < m && (ni >= k || w[li] <= w[ni])) ? li++ : ni++;
            up[take] = (uint16_t)k;
            sum += w[take];
        }
        w[k] = sum;
    }
    int count[B5H_MAXBITS + 1];
    for (int b = 0; b <= maxbits; b++) count[b] = 0;
    up[2 * m - 2] = 0;                                    // the root's depth
    for (int k = 2 * m - 3; k >= 0; k--) {                // a parent comes after its children: depths top down
        const uint16_t d = (uint16_t)(up[up[k]] + 1);
        up[k] = d;
        if (k < m) count[d < maxbits ? d : maxbits]++;
    }
    unsigned long long total = 0;
    for (int b = 1; b <= maxbits; b++) total += (unsigned long long)count[b] << (maxbits - b);
    while (total > (1ull << maxbits)) {
        count[maxbits]--;
        for (int b = maxbits - 1; b > 0; b--)
            if (count[b]) { count[b]--; count[b + 1] += 2; break; }
        total--;
    }
    int j = 0;
    for (int b = maxbits; b > 0; b--)
        for (int c = 0; c < count[b]; c++) len[sorted[j++]] = (uint8_t)b;
}

// step 6: code[s] = bit-reversed canonical code | len << 16
B5H_HD inline void b5h_codes(const uint8_t* len, int nsym, uint32_t* code) {
    uint32_t bl[B5H_MAXBITS + 1], next[B5H_MAXBITS + 1];
    for (int b = 0; b <= B5H_MAXBITS; b++) bl[b] = 0;
    for (int s = 0; s < nsym; s++) bl[len[s]]++;
    bl[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b <= B5H_MAXBITS; b++) { c = (c + bl[b - 1]) << 1; next[b] = c; }
    for (int s = 0; s < nsym; s++) {
        const int l = len[s];
        uint32_t v = 0;
        if (l) {
            const uint32_t x = next[l]++;
            for (int b = 0; b < l; b++) v |= ((x >> b) & 1u) << (l - 1 - b);
        }
        code[s] = v | (uint32_t)l << 16;
    }
}

// the run-length coding of lengths len[0..n) appended at rle[*nr]
B5H_HD inline void b5h_rle(const uint8_t* len, int n, uint16_t* rle, int* nr) {
    int i = 0;
    while (i < n) {
        const int v = len[i];
        int run = 1;
        while (i + run < n && len[i + run] == v) run++;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int k = run < 138 ? run : 138; rle[(*nr)++] = (uint16_t)(18 | (k - 11) << 8); run -= k; }
            if (run >= 3) { rle[(*nr)++] = (uint16_t)(17 | (run - 3) << 8); run = 0; }
            while (run > 0) { rle[(*nr)++] = 0; run--; }
        } else {
            rle[(*nr)++] = (uint16_t)v; run--;
            while (run >= 3) { const int k = run < 6 ? run : 6; rle[(*nr)++] = (uint16_t)(16 | (k - 3) << 8); run -= k; }
            while (run > 0) { rle[(*nr)++] = (uint16_t)v; run--; }
        }
    }
}

struct B5HBits {                          // LSB-first bit writer into bytes
    uint8_t* p; uint32_t n; uint32_t acc; int k;
    B5H_HD void put(uint32_t v, int nb) {
        acc |= v << k; k += nb;
        while (k >= 8) { p[n++] = (uint8_t)acc; acc >>= 8; k -= 8; }
    }
    B5H_HD uint32_t bits() const { return n * 8 + (uint32_t)k; }
    B5H_HD void finish() { if (k) p[n++] = (uint8_t)acc; }
};

// one block's code and header from its (prepared, step 1) frequencies and their order (step 2): fills *out, returns header + data bits
B5H_HD inline unsigned long long b5h_build(const uint32_t* freq, const uint16_t* sorted, int m, int maxbits, int final_block,
                                           B5HuffCode* out, B5HuffWork* wk) {
    for (int s = 0; s < B5H_SYMS; s++) wk->len[s] = 0;
    b5h_lengths(freq, sorted, m, maxbits, wk->len, wk->w, wk->up);
    b5h_codes(wk->len, B5H_SYMS, out->code);
    unsigned long long db = 0;
    for (int s = 0; s < B5H_SYMS; s++) db += (unsigned long long)freq[s] * wk->len[s];
    out->data_bits = db;
    // the header: literal lengths and distance lengths, run-length coded, then the code-length code over what that produced
    int nr = 0;
    b5h_rle(wk->len, B5H_SYMS, wk->rle, &nr);
    const uint8_t dist[2] = {1, 1};
    b5h_rle(dist, 2, wk->rle, &nr);
    for (int s = 0; s < 19; s++) { wk->clf[s] = 0; wk->cll[s] = 0; }
    for (int j = 0; j < nr; j++) wk->clf[wk->rle[j] & 0xff]++;
    const int cm = b5h_prepare(wk->clf, 19);
    b5h_sort(wk->clf, 19, wk->cls);
    b5h_lengths(wk->clf, wk->cls, cm, B5H_CL_MAXBITS, wk->cll, wk->w, wk->up);
    b5h_codes(wk->cll, 19, wk->clc);
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int ncl = 19;
    while (ncl > 4 && wk->cll[order[ncl - 1]] == 0) ncl--;
    B5HBits o{out->hdr, 0, 0, 0};
    o.put(final_block ? 1u : 0u, 1); o.put(2u, 2);       // BFINAL, BTYPE 10
    o.put(0u, 5); o.put(1u, 5); o.put((uint32_t)(ncl - 4), 4);
    for (int j = 0; j < ncl; j++) o.put(wk->cll[order[j]], 3);
    for (int j = 0; j < nr; j++) {
        const int s = wk->rle[j] & 0xff, x = wk->rle[j] >> 8;
        o.put(wk->clc[s] & 0xffffu, (int)(wk->clc[s] >> 16));
        if (s == 16) o.put((uint32_t)x, 2);
        else if (s == 17) o.put((uint32_t)x, 3);
        else if (s == 18) o.put((uint32_t)x, 7);
    }
    out->hdr_bits = o.bits();
    o.finish();
    out->pad_ = 0;
    return (unsigned long long)out->hdr_bits + db;
}
