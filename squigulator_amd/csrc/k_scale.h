// k_scale.h -- per-read sums of the caller's event rows and of the read's targets, and the shift / scale estimate from them (include/sqg_scale.h)
// Part of the device code of the per-read signal path; included through sqg_kernels.h behind k_collapse.h; the rows are k_rows.h's.
//
//   k_scale_sums<KIND>   a flat grid over the ROWS (SCL_ROWS, SCL_FIT) or over the batch's EVENTS (SCL_TARGETS: the same reduction, a read's
//                        events in place of its rows), one row per lane, 64 rows per wavefront trip.  The grid is CAPPED (h_scale.h:
//                        scale_grid) and loops: a wavefront owns `trips` CONSECUTIVE trips, not every gridDim-th one, so that its rows
//                        almost always belong to one read -- reads are long.  While a trip lies inside one read (one comparison against
//                        the end of the read the wavefront is in; a search in the offsets only when it fails) every lane adds its row to
//                        accumulators it keeps in registers over the trips; when the read changes, and at the end, the wavefront reduces
//                        them and lane 0 issues ONE set of 64-bit integer adds to the read's sums (profiles/pileup.md, profiles/collapse.md:
//                        a counter that every row hits is what to avoid).  A trip that holds a read boundary is combined by the run
//                        combination of k_rows.h (wave_runs, wave_run_part), a run being the lanes of one read, and the last lane of every run
//                        adds.  Integer adds commute: no sum depends on where the cuts fall or on arrival order.  No-return relaxed agent-scope atomics.
//                        The row value needs no 64-bit integer division: for |16 sum| < 2^52 the double quotient is within one of the
//                        floor and is corrected by the remainder; beyond, |16 sum / len| > 2^20 whatever len < 2^31 is, and the clamp decides.
//                        SCL_FIT gathers level_raw[ev[i]]: 2 B per row, any order of ev.
//   k_scale_derive<FIT>  one thread per read: the sums to the caller's arrays, gain / shift from them in FP64 as the header states them.
#pragma once

enum { SCL_N, SCL_SY, SCL_SYY, SCL_SX, SCL_SXX, SCL_SXY, SCL_DROP, SCL_COLS };      // the columns of ScaleParams.acc
enum { SCL_ROWS, SCL_TARGETS, SCL_FIT };                                             // k_scale_sums' kinds

struct ScaleParams {
    RowsIn rows;
    long long n_events;
    long long trips;                                          // 64-row trips a wavefront makes, one behind the other
    const long long *sum, *ev; const int* len;                // the caller's rows; ev: SCL_FIT only
    const int16_t* level_raw;                                 // [n_events] k_evtab_scan's column (scratch)
    unsigned long long* acc;                                  // [SCL_COLS][n_reads] scratch, zeroed
};

struct ScaleOut {                                             // the caller's, [n_reads], any may be null
    long long *n, *nx, *sy, *syy, *sx, *sxx, *sxy; int *gain, *shift, *rd_dropped;
};

// y of a row: clamp(floor(16 sum / max(len, 1)), -2^20, 2^20), the product modulo 2^64
__device__ __forceinline__ long long scale_row_value(const long long s, const int len) {
    const long long l = max(len, 1);
    const long long p = (long long)((unsigned long long)s << 4);
    if (p <= -(1LL << 52) || p >= (1LL << 52)) return p < 0 ? -(1LL << 20) : 1LL << 20;      // |p / l| > 2^21: l < 2^31
    long long q = (long long)floor((double)p / (double)l);                                   // (p and l are exact doubles; q is the floor or one off it)
    const long long rem = p - q * l;
    q += rem < 0 ? -1 : rem >= l ? 1 : 0;
    return min(max(q, -(1LL << 20)), 1LL << 20);
}

// what a kind sums: SCL_ROWS (sy, syy), SCL_TARGETS (sx, sxx), SCL_FIT every column; its k-th accumulator's column of acc
template <int KIND> __host__ __device__ constexpr int scale_cols() { return KIND == SCL_FIT ? 7 : 2; }
template <int KIND> __device__ __forceinline__ constexpr int scale_col(const int k) { return KIND == SCL_ROWS ? SCL_SY + k : KIND == SCL_TARGETS ? SCL_SX + k : k; }

// the wavefront's accumulators to read `cur` (none: -1), and zero again.  All 64 lanes call it.
template <int KIND>
__device__ __forceinline__ void scale_flush(const ScaleParams& P, unsigned long long (&a)[scale_cols<KIND>()], const int cur, const int lane) {
    if (cur < 0) return;                                                                      // (the same in every lane; a is zero)
#pragma unroll
    for (int k = 0; k < scale_cols<KIND>(); k++) {
        unsigned long long v = a[k];
#pragma unroll
        for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
        if (lane == 0 && v) __hip_atomic_fetch_add(P.acc + (long long)scale_col<KIND>(k) * P.rows.n_reads + cur, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a[k] = 0;
    }
}

template <int KIND>
__global__ __launch_bounds__(CHUNK_WG) void k_scale_sums(ScaleParams P) {
    constexpr int N = scale_cols<KIND>();
    const RowsIn& R = P.rows;
    const int lane = threadIdx.x & 63;
    const long long n = KIND == SCL_TARGETS ? P.n_events : R.n_rows;
    // the first row (SCL_TARGETS: event) of read r, r = n_reads: their number
    const auto off = [&](const int r) { return KIND != SCL_TARGETS ? R.row_off[r] : r < R.n_reads ? R.reads[r].ev_off : P.n_events; };
    const long long wave = (long long)blockIdx.x * (CHUNK_WG / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long span = 64 * P.trips;
    const long long end = min((wave + 1) * span, n);              // this wavefront's rows: [wave * span, end)
    unsigned long long a[N];
#pragma unroll
    for (int k = 0; k < N; k++) a[k] = 0;
    int cur = -1;                                                 // the read the accumulators belong to (the same in every lane)
    long long cur_end = 0; EventRange cur_ev{0, 0};               // the end of its rows; SCL_FIT: its events
    for (long long base = wave * span; base < end; base += 64) {
        const long long i = base + lane;
        const bool have = i < end;
        const long long w1 = min(base + 63, end - 1);             // the trip's last row
        bool one = cur >= 0 && w1 < cur_end;                      // the trip lies inside read `cur`
        int r = cur;
        if (!one) {
            const int r0 = rows_read_of(off, max(cur, 0), R.n_reads - 1, base);
            const int r1 = rows_read_of(off, r0, R.n_reads - 1, w1);
            scale_flush<KIND>(P, a, cur, lane);
            if (r0 == r1) {
                one = true; r = cur = r0; cur_end = off(r0 + 1);
                if (KIND == SCL_FIT) cur_ev = read_event_range(R.reads[r0]);
            } else {
                cur = -1;
                r = have ? rows_read_of(off, r0, r1, i) : r1;                                  // (the lanes behind the last row: the last run, zeros)
            }
        }
        unsigned long long t[N];
#pragma unroll
        for (int k = 0; k < N; k++) t[k] = 0;
        if (have) {
            if (KIND == SCL_TARGETS) {
                const long long x = 16 * (long long)P.level_raw[i];
                t[0] = (unsigned long long)x; t[1] = (unsigned long long)(x * x);
            } else if (KIND == SCL_ROWS) {
                const long long y = scale_row_value(P.sum[i], P.len[i]);
                t[0] = (unsigned long long)y; t[1] = (unsigned long long)(y * y);
            } else {
                const EventRange mine = one ? cur_ev : read_event_range(R.reads[r]);
                const long long e = P.ev[i];
                if (e >= mine.lo && e < mine.hi) {
                    const long long y = scale_row_value(P.sum[i], P.len[i]);
                    const long long x = 16 * (long long)P.level_raw[e];
                    t[0] = 1; t[1] = (unsigned long long)y; t[2] = (unsigned long long)(y * y);
                    t[3] = (unsigned long long)x; t[4] = (unsigned long long)(x * x); t[5] = (unsigned long long)(x * y);
                } else t[N - 1] = 1;
            }
        }
        if (one) {
#pragma unroll
            for (int k = 0; k < N; k++) a[k] += t[k];
            continue;
        }
        // a read boundary inside the trip (every lane of the wavefront is here): a run is the lanes of one read
        const int r_up = __shfl_up(r, 1, 64);
        const auto [first, tail] = wave_runs(lane == 0 || r != r_up, lane);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {                                                    // wave_run_scan's steps over the array
#pragma unroll
            for (int k = 0; k < N; k++) t[k] += wave_run_part(t[k], d, lane - d >= first);
        }
        if (tail) {
#pragma unroll
            for (int k = 0; k < N; k++)
                if (t[k]) __hip_atomic_fetch_add(P.acc + (long long)scale_col<KIND>(k) * R.n_reads + r, t[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    scale_flush<KIND>(P, a, cur, lane);
}

// gain (Q16) and shift (1/256 code) from a read's sums: include/sqg_scale.h's expressions, one rounding per operation (the build has
// -ffp-contract=off; double division and sqrt are correctly rounded on this device: k_events_table.h)
template <bool FIT>
__device__ __forceinline__ void scale_estimate(const long long n, const long long nx, const long long sy, const long long syy, const long long sx,
                                               const long long sxx, const long long sxy, int* gain, int* shift) {
    *gain = 65536; *shift = 0;
    if (n == 0 || nx == 0) return;
    const double dn = (double)n, dnx = (double)nx;
    const double my = (double)sy / dn, mx = (double)sx / dnx;
    const double ey = (double)syy / dn, ex = (double)sxx / dnx;
    const double my2 = my * my, mx2 = mx * mx;
    const double vy = ey - my2, vx = ex - mx2;
    double g = 1.0;
    if (FIT) {
        const double exy = (double)sxy / dn;
        const double mxy = mx * my;
        const double cxy = exy - mxy;
        if (vy > 0) g = cxy / vy;
    } else if (vy > 0 && vx > 0) g = sqrt(vx / vy);
    g = g < 1.0 / 65536.0 ? 1.0 / 65536.0 : g;
    g = g > 16.0 ? 16.0 : g;
    const double gm = g * my;
    const double s = mx - gm;
    double sh = rint(s * 16.0);
    sh = sh < -67108864.0 ? -67108864.0 : sh;
    sh = sh > 67108864.0 ? 67108864.0 : sh;
    *gain = (int)rint(g * 65536.0);
    *shift = (int)sh;
}

// no_rows: the call has no row at all, and every sum is 0 (the header's n_rows == 0)
template <bool FIT>
__global__ __launch_bounds__(CHUNK_WG) void k_scale_derive(ScaleParams P, ScaleOut O, int no_rows) {
    const int r = blockIdx.x * CHUNK_WG + threadIdx.x;
    const RowsIn& R = P.rows;
    if (r >= R.n_reads) return;
    const auto col = [&](const int c) { return (long long)P.acc[(long long)c * R.n_reads + r]; };
    const ReadDesc rd = R.reads[r];
    const long long n = FIT ? col(SCL_N) : R.row_off[r + 1] - R.row_off[r];
    const long long nx = FIT ? n : no_rows ? 0 : read_events(rd);
    const long long sy = col(SCL_SY), syy = col(SCL_SYY), sx = col(SCL_SX), sxx = col(SCL_SXX), sxy = col(SCL_SXY);
    int gain, shift;
    scale_estimate<FIT>(n, nx, sy, syy, sx, sxx, sxy, &gain, &shift);
    if (O.n) O.n[r] = n;
    if (O.nx) O.nx[r] = nx;
    if (O.sy) O.sy[r] = sy;
    if (O.syy) O.syy[r] = syy;
    if (O.sx) O.sx[r] = sx;
    if (O.sxx) O.sxx[r] = sxx;
    if (O.sxy) O.sxy[r] = sxy;
    if (O.gain) O.gain[r] = gain;
    if (O.shift) O.shift[r] = shift;
    if (O.rd_dropped) O.rd_dropped[r] = (int)col(SCL_DROP);
}
