// el_cell.h — the ersatz-material value of a cell from ϕ, one definition for lsm_elliptic.hip (the cell coefficient a) and
// lsm_elastic.hip (the cell modulus E): both files are built without contraction, so the two cell arrays of one ϕ have the same bits.
#pragma once
#include "lsm_handle.h"

namespace lsm {

// at: the padded index of the cell's lowest corner; s1, s2: the field's strides.  mean = (Σ corners in ascending linear index)·2^−N;
// θ = clamp(½ − (mean − level)/hmin, 0, 1); the value is v_out + (v_in − v_out)·θ
template <int N>
__device__ __forceinline__ double el_cell_from_phi(const void* __restrict__ phi, long long at, long long s1, long long s2, int f32, double level, double v_in,
                                                   double v_out, double hmin) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {    // the corners in ascending linear index
        const long long o = (m & 1) + ((m >> 1) & 1) * s1 + (N > 2 ? ((m >> 2) & 1) * s2 : 0);
        const double p = ld_val(phi, at + o, f32);
        s = m == 0 ? p : s + p;
    }
    const double mean = s * (N == 2 ? 0.25 : 0.125);
    const double theta = fmin(fmax(0.5 - (mean - level) / hmin, 0.0), 1.0);
    return v_out + (v_in - v_out) * theta;
}

}  // namespace lsm
