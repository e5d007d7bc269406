// k_detect.h -- the two-window t-statistic event detector on a batch's stored signal (include/sqg_detect.h): the boundaries, then the rows between them
// Part of the device code of the per-read signal path; included through sqg_kernels.h behind k_pileup.h.
//
//   k_detect_walk<FILL>  the peak machine is a serial chain along a read whose result must not depend on how the work is cut, so the work is
//                        cut ACROSS reads: one read per lane, one wavefront per workgroup.  The wavefront loads a tile of DET_T samples of
//                        each of its 64 reads, with a halo of DET_H (the largest window) on either side, coalesced into LDS -- a row per
//                        read, samples outside the read as zeros --, then every lane walks its own row: the six window sums slide by one
//                        add and one subtract per sample in integers (no prefix array), both statistics are taken for DET_U samples at
//                        once ahead of the machines (a wavefront has its SIMD to itself, and the divisions and square roots of
//                        neighbouring samples are all it has to overlap: 8 % on the headline batch, profiles/detect.md), and the
//                        machine's state lives in registers from tile to tile: a peak found in one tile is recorded in the next.  The lengths of a wavefront's
//                        reads differ, so every lane has its own bounds; a lane whose read has ended idles until the longest read of
//                        its wavefront has.  The row stride is an odd number of dwords: the lanes read the same column of their own rows,
//                        and the 32 rows of a half wavefront then lie in 32 different banks.  The launch lasts as long as the longest
//                        read of the batch: that, not memory, bounds it (profiles/detect.md).
//                        FILL = false counts every read's rows (the plan); FILL = true runs the same machine again and writes dt_start /
//                        dt_read at the plan's offsets.
//   k_detect_rows<PA>    a flat grid over the batch's detected rows, one row per lane: k_events_table.h's reduction (evtab_take) and
//                        mean / sd (evtab_derive) with the row's length from the next boundary instead of the dwells, and true_ev by one
//                        binary search in the ev_start column k_evtab_scan wrote.
#pragma once

#define DET_T 256                                    // samples of a tile
#define DET_H 64                                     // halo on either side: the largest w_long (include/sqg_detect.h)
#define DET_STRIDE (DET_T + 2 * DET_H + 2)           // int16 per LDS row: 193 dwords, odd
#define DET_U 4                                      // samples whose statistics a lane takes at once, ahead of its machines; divides DET_T

struct DetectParams {
    BatchView bv;
    int w[2];                                        // w_short, w_long
    double th[2], h;                                 // thr_short, thr_long; peak_height
    int* count;                                      // [n_reads] rows of every read (FILL = false)
    const long long* det_off;                        // [n_reads+1] first row of every read (FILL = true)
    long long* dt_start; int* dt_read;               // [n_rows] the caller's or scratch (FILL = true): never null then
};

// the sums of one window at position i, samples outside the read counting as zeros: S1 over [i-w, i), S2 over [i, i+w), Q of the squares over both
// (Q in a double: an integer below 2^37, exact)
struct DetWin { int s1, s2; double q; };

// t_w[i] of include/sqg_detect.h from the window's sums.  The header's integers are formed in doubles: every product and difference below
// is an integer under 2^53, so none of them rounds, and the one division and the one square root round once each (-ffp-contract=off; both
// correctly rounded on this device, as evtab_derive relies on).  No 64-bit integer multiply, no 64-bit conversion.
__device__ __forceinline__ double detect_t(const double w, const DetWin& A) {
    const double s1 = (double)A.s1, s2 = (double)A.s2, d = s2 - s1;              // |s1|, |s2| <= 2^21
    const double N = w * (d * d);                                                // < 2^51
    const double D = w * A.q - s1 * s1 - s2 * s2;                                // 0 <= D < 2^44
    return sqrt(N / (D > 0 ? D : 1.0));
}

template <bool FILL>
__global__ __launch_bounds__(64) void k_detect_walk(DetectParams P) {
    __shared__ int16_t tile[64 * DET_STRIDE];
    const BatchView& V = P.bv;
    const int lane = threadIdx.x;
    const int r0 = blockIdx.x * 64;
    const int nr = min(64, V.n_reads - r0);                       // reads of this wavefront (at least 1)
    const bool have = lane < nr;
    const long long n = have ? V.sig_off[r0 + lane + 1] - V.sig_off[r0 + lane] : 0;
    long long n_max = n;
#pragma unroll
    for (int d = 32; d; d >>= 1) n_max = max(n_max, __shfl_xor(n_max, d, 64));
    const int w0 = P.w[0], w1 = P.w[1];
    const double dw0 = (double)w0, dw1 = (double)w1;
    const double th0 = P.th[0], th1 = P.th[1], h = P.h;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    // the two machines and what they share
    long long pos[2] = {-1, -1}, masked[2] = {0, 0}, last = 0;
    double val[2] = {inf, inf};
    bool valid[2] = {false, false};
    DetWin A[2] = {{0, 0, 0}, {0, 0, 0}};
    long long rows = n > 0 ? 1 : 0;
    const long long out0 = FILL && have ? P.det_off[r0 + lane] : 0;
    const long long room = FILL && have ? P.det_off[r0 + lane + 1] - out0 : 0;       // the plan's rows: the same machine gives no more, and nothing is written past them
    if (FILL && room > 0) { P.dt_start[out0] = 0; P.dt_read[out0] = r0 + lane; }
    const int16_t* row = tile + lane * DET_STRIDE;
    for (long long t0 = 0; t0 < n_max; t0 += DET_T) {
        __syncthreads();                                          // (the walk of the tile before)
        // the tile: samples [t0 - DET_H, t0 + DET_T + DET_H) of every read that still has some, zeros where the read has none.  j, and
        // with it the read's bounds, is the same in every lane.
        for (int j = 0; j < nr; j++) {
            const long long base = V.sig_off[r0 + j];
            const long long nj = V.sig_off[r0 + j + 1] - base;
            if (nj <= t0) continue;                               // (its lane walks no more)
            int16_t* dst = tile + j * DET_STRIDE;
            for (int c = lane; c < DET_T + 2 * DET_H; c += 64) {
                const long long p = t0 - DET_H + c;
                dst[c] = p >= 0 && p < nj ? V.sig[base + p] : (int16_t)0;
            }
        }
        __syncthreads();
        if (t0 == 0 && have) {                                    // the sums at i = 0: nothing in front, the first w samples behind
#pragma unroll
            for (int k = 0; k < 2; k++)
                for (int j = 0; j < P.w[k]; j++) { const int x = row[DET_H + j]; A[k].s2 += x; A[k].q += (double)(x * x); }
        }
        const int steps = (int)min((long long)DET_T, n - t0);     // this lane's own bound; <= 0: its read has ended
        for (int s = 0; s < steps; s += DET_U) {
            // the statistics of the next DET_U samples, both windows: the sums slide whatever the machines do, so these 2 DET_U divisions
            // and square roots are independent of one another and overlap; the machines, a chain of compares, follow.  (A read that ends
            // inside the group slides over the zeros behind it: DET_T is a multiple of DET_U, the columns stay inside the row.)
            double t[DET_U][2];
#pragma unroll
            for (int u = 0; u < DET_U; u++) {
                const long long i = t0 + s + u;
                const int c = DET_H + s + u;                      // x[i]'s column
                const int x0 = row[c];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int w = k ? w1 : w0;
                    const double tk = detect_t(k ? dw1 : dw0, A[k]);
                    t[u][k] = i < w || i > n - w ? 0.0 : tk;
                    const int xm = row[c - w], xp = row[c + w];   // slide to i + 1
                    A[k].s1 += x0 - xm; A[k].s2 += xp - x0; A[k].q += (double)(xp * xp - xm * xm);
                }
            }
#pragma unroll
            for (int u = 0; u < DET_U; u++) {
                const long long i = t0 + s + u;
                if (s + u >= steps) break;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (masked[k] >= i) continue;
                    const int w = k ? w1 : w0;
                    const double thk = k ? th1 : th0;
                    const double cur = t[u][k];
                    if (pos[k] < 0) {
                        if (cur < val[k]) val[k] = cur;
                        else if (cur - val[k] > h) { val[k] = cur; pos[k] = i; }
                    } else {
                        if (cur > val[k]) { val[k] = cur; pos[k] = i; }
                        if (k == 0 && val[0] > th0) { masked[1] = pos[0] + w0; pos[1] = -1; val[1] = inf; valid[1] = false; }
                        if (val[k] - cur > h && val[k] > thk) valid[k] = true;
                        if (valid[k] && i - pos[k] > w / 2) {
                            if (pos[k] > last) {
                                if (FILL && rows < room) { P.dt_start[out0 + rows] = pos[k]; P.dt_read[out0 + rows] = r0 + lane; }
                                rows++;
                                last = pos[k];
                            }
                            pos[k] = -1; val[k] = cur; valid[k] = false;
                        }
                    }
                }
            }
        }
    }
    if (!FILL && have) P.count[r0 + lane] = (int)rows;
}

struct DetectRowParams {
    const long long* det_off;                        // [n_reads+1]
    long long n_rows;
    const long long* dt_start; const int* dt_read;   // the caller's or scratch: never null
    int* dt_len; long long* true_ev;                 // the caller's, may be null
    const long long* ev_start;                       // [n_events] k_evtab_scan's column; null when true_ev is
};

// Row i of a flat grid over the batch's detected rows: evtab_event's sibling, the length from the next boundary (or the read's end)
// instead of the dwells
__device__ __forceinline__ EventAt detect_row(const DetectRowParams& U, const BatchView& V, const long long i) {
    const int r = U.dt_read[i];
    const long long s = U.dt_start[i];
    const long long end = i + 1 < U.det_off[r + 1] ? U.dt_start[i + 1] : V.sig_off[r + 1] - V.sig_off[r];
    return {r, (int)(end - s), V.sig_off[r] + s};
}

// The event of read r that holds stored sample s: its ev_start is at most s and the next one's (in stored order) above s.  ev_start
// ascends along a DNA read's events and descends along an RNA read's; an event without samples shares its ev_start with the one behind
// it in stored order and is never the answer.
__device__ __forceinline__ long long detect_true_ev(const long long* ev_start, const ReadDesc& rd, const bool rna, const long long s) {
    long long lo = rd.ev_off, hi = rd.ev_off + rd.ne0 + max(rd.ne1, 0);          // [lo, hi)
    if (!rna) {                                                   // the last event with ev_start <= s
        while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (ev_start[mid] <= s) lo = mid; else hi = mid; }
        return lo;
    }
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (ev_start[mid] <= s) hi = mid; else lo = mid + 1; }      // the first one
    return lo;
}

template <bool PA>
__global__ __launch_bounds__(CHUNK_WG) void k_detect_rows(EventParams Q, DetectRowParams U) {
    const uint32_t* W = reinterpret_cast<const uint32_t*>(Q.bv.sig);
    evtab_for_rows(U.n_rows, [&](const long long i, const bool have, const int lane) {
        const auto [r, len, s0] = have ? detect_row(U, Q.bv, i) : EventAt{0, 0, 0};
        const bool reduce = Q.sum || Q.sumsq || Q.vmin || Q.vmax || Q.mean || Q.sd;      // (the same in every lane)
        const EventAcc A = reduce ? evtab_take(W, have, len, s0, lane) : EventAcc{0, 0, 0, 0};
        if (!have) return;
        if (U.dt_len) U.dt_len[i] = len;
        if (U.true_ev) U.true_ev[i] = detect_true_ev(U.ev_start, Q.bv.reads[r], Q.bv.rna, s0 - Q.bv.sig_off[r]);
        evtab_store<PA>(Q, i, r, len, A);
    });
}
