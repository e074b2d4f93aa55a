// Test plug-in: one user-compiled device Calculator that uses every facility mcmcpp_amd/csrc/mcmcpp_hip_plugin.hpp names.
//   coupled_table  a Gaussian with nearest-neighbour and mirror coupling, params = {mu[D], w[D], c[D], r} (3 D + 1 elements):
//                  with d_j = x_j - mu_j, every operation rounded on its own,
//                      a_j = w_j (d_j d_j),  b_j = c_j (d_j d_{j+1}) for j + 1 < D,  m_j = r (d_j d_{D-1-j}),
//                      t_j = (a_j + b_j) + m_j  (a_j + m_j at j = D - 1),  logp = -1/2 tree_sum(t)
//                  (oracle/stretch_oracle.h: SO_CALC_COUPLED_TABLE is the same sum as a plain loop over j)
// Where each input comes from is the point of this functor (tests/test_plugin_contract.py):
//   mu, w  the block-shared table: block_commit copies params[0 .. 2 D) to LDS, eval reads them from g.block_scratch only
//   c      registers of the functor's own: preload loads this lane's slice of params + 2 D into Regs, eval reads c only from there
//   r      params[3 D], read in eval
//   d      formed in registers, published to the wave-private stage; d_{j+1} (the neighbouring lane's, for a lane's last
//          element) and d_{D-1-j} (anywhere in the group) are read back through g.element()
#include "mcmcpp_hip_plugin.hpp"

template <class T>
struct CoupledTable
{
    static constexpr bool kNeedsStage = true;
    template <int EPL, int LPW>
    struct MatrixCore
    {
        static constexpr bool kUse = false;
    };
    __host__ __device__ static size_t block_scratch_elems(int D) { return 2 * (size_t)D; }
    struct Prefetch
    {
    };
    __device__ static void block_prefetch(Prefetch&, const T*, int, bool, int, int) {}
    __device__ static void block_commit(const Prefetch&, T* scratch, const T* prm, int D, bool, int tid, int nthreads)
    {
        for (int k = tid; k < 2 * D; k += nthreads) scratch[k] = prm[k];
    }
    template <int EPL, int LPW>
    struct Regs
    {
        T c[EPL];
    };
    template <int EPL, int LPW>
    __device__ static void preload(const mcmcpp::GroupCtx<T, EPL, LPW>& g, const T* prm, Regs<EPL, LPW>& regs)
    {
        const int D = g.dims, i0 = g.first_index();
#pragma unroll
        for (int e = 0; e < EPL; ++e) regs.c[e] = (i0 + e < D) ? prm[2 * D + i0 + e] : (T)0;
    }
    template <int EPL, int LPW>
    __device__ static T eval(const mcmcpp::GroupCtx<T, EPL, LPW>& g, const T* prm, const Regs<EPL, LPW>& regs, const T (&x)[EPL])
    {
        const int D = g.dims, i0 = g.first_index();
        const T* mu = g.block_scratch;
        const T* w = g.block_scratch + D;
        T d[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) d[e] = (i0 + e < D) ? x[e] - mu[i0 + e] : (T)0;
        g.publish(d);
        const T r = prm[3 * D];
        T t[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e)
        {
            const int j = i0 + e;
            T term = (T)0;
            if (j < D)
            {
                const T dd = d[e] * d[e];
                const T a = w[j] * dd;
                const T dm = g.element(D - 1 - j);
                const T pm = d[e] * dm;
                const T m = r * pm;
                if (j + 1 < D)
                {
                    const T dn = g.element(j + 1);
                    const T pn = d[e] * dn;
                    const T b = regs.c[e] * pn;
                    const T ab = a + b;
                    term = ab + m;
                }
                else
                    term = a + m;
            }
            t[e] = term;
        }
        return (T)-0.5 * g.tree_sum(t);
    }
};

MCMCPP_HIP_PLUGIN_CALCULATOR(CoupledTable, coupled_table)
