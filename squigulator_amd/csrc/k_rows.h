// k_rows.h -- what the kernels that take the caller's rows share (include/sqg_align.h, sqg_collapse.h, sqg_scale.h): the rows as a kernel
// gets them (RowsIn), a row's value (rows_q), the read of a row (rows_read_of) and the wavefront's run combination (wave_runs, wave_run_scan), whose method
// k_collapse.h describes.  Part of the device code of the per-read signal path; included through sqg_kernels.h in front of k_align.h.
#pragma once

struct RowsIn {
    const ReadDesc* reads;                                    // [n_reads]: a read's events are read_event_range()
    const long long* row_off;                                 // [n_reads+1] device copy of the caller's
    int n_reads; long long n_rows;
};

// q of a row (include/sqg_scale.h): q0 = floor(256 * sum / max(len, 1)), the product modulo 2^64, clamped to +-2^26; SCALED: ((gain * q0) >> 16) + off,
// clamped again (gain and off already clamped into their ranges by the caller: |gain q0| <= 2^46; >> of a negative: arithmetic, a floor)
template <bool SCALED>
__device__ __forceinline__ int rows_q(const long long s, const int len, const long long gain, const long long off) {
    const long long n = max(len, 1);
    const long long p = (long long)((unsigned long long)s << 8);
    long long q = p / n;
    if (p % n != 0 && p < 0) q--;                             // floor
    q = min(max(q, -(1LL << 26)), 1LL << 26);
    if (SCALED) q = min(max(((gain * q) >> 16) + off, -(1LL << 26)), 1LL << 26);
    return (int)q;
}

// the read of row i: the last r in [lo, hi] whose first row, off(r), is <= i (reads without rows are stepped over; off(lo) <= i is given)
template <class Off>
__device__ __forceinline__ int rows_read_of(const Off& off, int lo, int hi, const long long i) {
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off(mid) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the run of a lane from the heads of the wavefront (lane 0 is one; all 64 lanes call it): its first lane, and whether this lane is its last
struct WaveRun { int first; bool tail; };
__device__ __forceinline__ WaveRun wave_runs(const bool head, const int lane) {
    const unsigned long long heads = __ballot(head);
    return {63 - __builtin_clzll(heads & (~0ull >> (63 - lane))), lane == 63 || (((heads >> 1) >> lane) & 1ull)};
}

// The segmented scan: every lane adds to its values what its run holds in the lanes below it, so a run's last lane has the run's sums.
// wave_run_part is one of its six steps for one value: what the lane d below holds, 0 where that lane is outside the run.  A kernel with
// its values in an array (k_scale_sums) writes the two loops around it itself: the array by reference costs registers (profiles/rows_refactor.md).
template <class T>
__device__ __forceinline__ T wave_run_part(const T v, const int d, const bool inside) {
    const T u = __shfl_up(v, d, 64);
    return inside ? u : T(0);
}
template <class... T>
__device__ __forceinline__ void wave_run_scan(const int first, const int lane, T&... v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) ((v += wave_run_part(v, d, lane - d >= first)), ...);
}
