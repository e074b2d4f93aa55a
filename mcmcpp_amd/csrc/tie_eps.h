/* tie_eps.h -- the width of the near-tie band of the accept test, one definition for the device library and the oracle.
 *
 * Both sides decide `ln U < (D-1) ln z + logp_new - logp_old` (stretch move; differential evolution has no ln z term)
 * with logarithm functions of their own and count a decision as a near tie when
 *     |ln U - delta| <= tie_eps * (|ln U| + |(D-1) ln z| + |logp_new| + |logp_old|).
 * A decision can differ between the two sides only inside that band, provided (d + 3) * eps <= tie_eps, where d is the
 * distance in ulp between the two logarithms and eps is 2^-52 / 2^-23 (derivation and measured d: tests/test_accept_logs.py,
 * DESIGN.md section 8).  The two values must therefore be the same numbers on both sides.
 *
 * Plain C: included by sampler_host.hpp, diffevo.hip and oracle/stretch_oracle.c. */
#ifndef MCMCPP_TIE_EPS_H
#define MCMCPP_TIE_EPS_H

#define MCMCPP_TIE_EPS_F64 1e-12
#define MCMCPP_TIE_EPS_F32 6e-7f

#endif
