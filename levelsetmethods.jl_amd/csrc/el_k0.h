// el_k0.h — the host code that lsm_elastic.hip defines and lsm_homog.hip uses as well: the unit element matrix of a level and the
// symbol bound its damping comes from.  One definition, so the two operators hold the same K0 bits and the same ω.
#pragma once
#include <vector>

namespace lsm {

// the unit element matrix of a box cell with sides h, scaled by 1/∏h (include/lsm.h, "elasticity_solve"): (2^N·N)² doubles, row-major
void es_k0(int N, const double h[3], double lam, double mu, std::vector<double>& K);
// λmax(D⁻¹A) of the level's operator on a uniform infinite grid, from K0 alone
double es_symbol_lambda(int N, const std::vector<double>& K);

}  // namespace lsm
