// scan.h — the scan of the chunk sums, one definition: every feature that emits a result of variable length counts per chunk of
// 4096 items, scans the chunk counts here in ONE workgroup, reads the totals and writes at the scanned offsets (isosurface and
// volume_mesh: three rows; quadrature: two; components and nucleation: one).  Integer sums: any order gives the same.
//   * the rows are scanned one after the other (one row's registers at a time), each in rounds of 8 · 1024 values: thread t takes
//     the 8 consecutive values from base + 8t, and the sum of the rounds before is carried in a register of every thread;
//   * the scan of the 1024 thread sums of a round is wave.h's block_excl_scan<16>: one barrier per round.  Its LDS words come in
//     two sets that alternate by round, across the rows too: the barrier of round k + 1 lies between the reads of round k and the
//     writes of round k + 2;
//   * a thread reads only its own 8 positions and writes them only after it has read them into registers, and nobody else reads
//     or writes those: a row may be scanned in place (out == (Out*)in) where Out has 32 bits.
#pragma once
#include "wave.h"

namespace lsm {

constexpr int SCAN_THREADS = 1024, SCAN_PER = 8;

// per row: n values in, their exclusive scan out; nonzero: the scan is of in[i] != 0
template <class Out>
struct ScanRow {
    const unsigned* in;
    Out* out;
    int nonzero;
};
template <int ROWS, class Out>
struct ScanRows {
    ScanRow<Out> row[ROWS];
};

// out[i] := in[0] + … + in[i − 1] for every row, i < n; tot[r] := row r's total (0 where n == 0).  One workgroup.
template <int ROWS, class Out, class Tot>
__global__ void __launch_bounds__(SCAN_THREADS) chunk_scan_kernel(ScanRows<ROWS, Out> rows, long long n, Tot* tot) {
    __shared__ Out wsum[2][SCAN_THREADS / 64];
    int set = 0;
#pragma unroll 1
    for (int r = 0; r < ROWS; ++r) {
        const ScanRow<Out> row = rows.row[r];
        Out carry = 0;
        for (long long base = 0; base < n; base += SCAN_PER * SCAN_THREADS, set ^= 1) {      // uniform over the workgroup
            const long long i0 = base + (long long)SCAN_PER * threadIdx.x;
            unsigned v[SCAN_PER];
            Out acc = 0;
#pragma unroll
            for (int e = 0; e < SCAN_PER; ++e) {
                const unsigned x = i0 + e < n ? row.in[i0 + e] : 0u;
                v[e] = row.nonzero ? (x != 0u ? 1u : 0u) : x;
                acc += v[e];
            }
            Out total;
            Out p = carry + block_excl_scan<SCAN_THREADS / 64>(acc, wsum[set], total);
#pragma unroll
            for (int e = 0; e < SCAN_PER; ++e) {
                if (i0 + e < n) row.out[i0 + e] = p;
                p += v[e];
            }
            carry += total;
        }
        if (threadIdx.x == 0) tot[r] = (Tot)carry;
    }
}

template <int ROWS, class Out, class Tot>
inline void chunk_scan(hipStream_t stream, const ScanRows<ROWS, Out>& rows, long long n, Tot* tot) {
    hipLaunchKernelGGL((chunk_scan_kernel<ROWS, Out, Tot>), dim3(1), dim3(SCAN_THREADS), 0, stream, rows, n, tot);
}

}  // namespace lsm
