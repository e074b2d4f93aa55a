/*
 * stretch_oracle_typed.inc -- element-type-generic part of the oracle (included twice by
 * stretch_oracle.c with REAL = double / float).  TEST INFRASTRUCTURE ONLY.
 */

/* Canonical pairwise (binary-tree) sum over t[0..D): pad to the next power of two with +0 and add
 * halves recursively.  This is the summation order every built-in Calculator of this repo uses on
 * host and device alike (it does not depend on how a walker is spread over GPU lanes). */
static REAL SFX(tree_sum)(const REAL* t, int lo, int len, int D)
{
    if (len == 1) return lo < D ? t[lo] : (REAL)0;
    int h = len >> 1;
    return SFX(tree_sum)(t, lo, h, D) + SFX(tree_sum)(t, lo + h, h, D);
}

static int SFX(pow2_at_least)(int D)
{
    int n = 1;
    while (n < D) n <<= 1;
    return n;
}

/* The Calculator concept of the reference: ParamType calcLogPostProb(ParamType*)
 * (MCMCpp/Utility/UserOjbectsTest.h:77-79, Movers/StretchMove.h:47-53,111). */
static REAL SFX(calc_logp)(int calc_id, int D, const REAL* prm, const REAL* x)
{
    REAL t[D > 0 ? D : 1];
    int n2 = SFX(pow2_at_least)(D);
    switch (calc_id) {
    case SO_CALC_ISO_GAUSSIAN:
        for (int j = 0; j < D; ++j) t[j] = x[j] * x[j];
        return (REAL)-0.5 * SFX(tree_sum)(t, 0, n2, D);
    case SO_CALC_DENSE_GAUSSIAN:
        for (int i = 0; i < D; ++i) {
            REAL acc = (REAL)0;
            for (int j = 0; j < D; ++j) acc = FMA(prm[(size_t)i * D + j], x[j], acc);
            t[i] = x[i] * acc;
        }
        return (REAL)-0.5 * SFX(tree_sum)(t, 0, n2, D);
    case SO_CALC_ROSENBROCK: {
        const REAL a = prm[0], b = prm[1], c = prm[2];
        for (int i = 0; i < D; ++i) {
            if (i + 1 < D) {
                REAL u = x[i + 1] - x[i] * x[i];
                REAL v = a - x[i];
                t[i] = b * (u * u) + v * v;
            } else {
                t[i] = (REAL)0;
            }
        }
        return -(SFX(tree_sum)(t, 0, n2, D) * c);
    }
    case SO_CALC_SKEWED_GAUSSIAN_2D: {
        /* test/sequential/SkewedGaussian/Common/SkewedGaussian.h:52-57, same operation order */
        const REAL eps = prm[0];
        REAL t1 = x[0] / (REAL)2 - x[1];
        REAL t2 = x[0] / (REAL)2 + x[1];
        return (((t1 * t1) / eps) + (t2 * t2)) / (REAL)-2;
    }
    case SO_CALC_BOXED_ISO_GAUSSIAN: {
        /* test target with a bounded support: the isotropic Gaussian's bits inside the box, prm[1] verbatim outside.
         * A NaN coordinate fails the comparison, so it is outside. */
        for (int j = 0; j < D; ++j)
            if (!(FABS(x[j]) <= prm[0])) {
#pragma omp atomic
                ++boxed_outside_evals;
                return prm[1];
            }
        for (int j = 0; j < D; ++j) t[j] = x[j] * x[j];
        return (REAL)-0.5 * SFX(tree_sum)(t, 0, n2, D);
    }
    case SO_CALC_COUPLED_TABLE: {
        /* test target: a Gaussian with nearest-neighbour and mirror coupling, prm = {mu[D], w[D], c[D], r}; every
         * operation rounded on its own, in the order written (stretch_oracle.h) */
        const REAL *mu = prm, *w = prm + D, *c = prm + 2 * (size_t)D;
        const REAL r = prm[3 * (size_t)D];
        for (int j = 0; j < D; ++j) {
            const REAL d = x[j] - mu[j];
            const REAL dm = x[D - 1 - j] - mu[D - 1 - j];
            const REAL a = w[j] * (d * d);
            const REAL m = r * (d * dm);
            if (j + 1 < D) {
                const REAL dn = x[j + 1] - mu[j + 1];
                const REAL b = c[j] * (d * dn);
                t[j] = (a + b) + m;
            } else {
                t[j] = a + m;
            }
        }
        return (REAL)-0.5 * SFX(tree_sum)(t, 0, n2, D);
    }
    default: return (REAL)0;
    }
}

/* The near-tie rule (stretch_oracle.h: so_near_ties): inside the band, and the margin finite. */
static int SFX(near_tie)(REAL margin, REAL band)
{
    return margin <= band && margin < (REAL)INFINITY;
}

/* One StretchMove::updateWalker (MCMCpp/Movers/StretchMove.h:100-123) given the three raw draws.
 * Returns 1 when the proposal was accepted.  `row_out`, when not NULL, receives the walker's
 * position after the update (Walker.h:105,172-179 -> ChainBlock.h:125-131). */
static int SFX(update_walker)(so_sampler* s, REAL* cur, REAL* cur_lp, const REAL* other, int n,
                              uint64_t r0, uint64_t r1, uint64_t r2, REAL* row_out, uint64_t* ties)
{
    const int D = s->cfg.num_params;
    REAL prop[D];
    /* StretchMove.h:102  partner = engine(n)  (pcg bounded_rand: r % n once r >= threshold) */
    const REAL* sel = other + (size_t)(r0 % (uint64_t)n) * D;
    /* StretchMove.h:104 + GwDistribution.h:45-58 */
    const REAL alpha = (REAL)(s->cfg.gw_alpha_num > 0 ? s->cfg.gw_alpha_num : 2) /
                       (REAL)(s->cfg.gw_alpha_den > 0 ? s->cfg.gw_alpha_den : 1);
    const REAL sqrt_a = SQRT(alpha);
    const REAL inv_sqrt_a = (REAL)1 / sqrt_a;
    const REAL term1 = sqrt_a - inv_sqrt_a;
    REAL u1 = CANON(r1);
    REAL tmp = term1 * u1 + inv_sqrt_a;
    REAL z = tmp * tmp;
    /* StretchMove.h:105-108 */
    for (int j = 0; j < D; ++j) prop[j] = sel[j] + z * (cur[j] - sel[j]);
    /* StretchMove.h:110-112 */
    REAL zs = LOG(z) * (REAL)(D - 1);
    REAL new_lp = SFX(calc_logp)(s->cfg.calc_id, D, (const REAL*)s->params, prop);
    REAL delta = zs + new_lp - *cur_lp;
    /* StretchMove.h:113: -expDist(engine) = -(-log(1 - u)/1)  (bits/random.h:4761-4767) */
    REAL u2 = CANON(r2);
    REAL ln_u = -(-LOG((REAL)1 - u2) / (REAL)1);
    int accept = ln_u < delta;
    {
        REAL margin = FABS(ln_u - delta);
        REAL scale = FABS(ln_u) + FABS(zs) + FABS(new_lp) + FABS(*cur_lp);
        if (SFX(near_tie)(margin, (REAL)TIE_EPS * scale)) {
            ++*ties;
#pragma omp critical(so_tie_record)
            {
                s->tie_half_step = s->half_steps;
                s->tie_walker = (uint32_t)((size_t)(cur - (REAL*)s->pos) / (size_t)D);
                s->tie_accepted = accept;
                s->tie_ln_u = (double)ln_u;
                s->tie_delta = (double)delta;
            }
        }
    }
    if (accept) {
        memcpy(cur, prop, sizeof(REAL) * (size_t)D);
        *cur_lp = new_lp;
    }
    if (row_out) memcpy(row_out, cur, sizeof(REAL) * (size_t)D);
    return accept;
}

/* One half of EnsembleSampler::performStep (EnsembleSampler.h:345-354): every walker of `color`
 * (0 = red = walkers [0,n), 1 = black = [n,2n)) is updated against the other half as it stands.
 * `eng` is the engine positioned at this half-step's first draw; it leaves positioned at the next. */
static uint32_t SFX(half_step)(so_sampler* s, int color, REAL* chain_step, int mode, int threads,
                               so_pcg64* eng)
{
    const int D = s->cfg.num_params;
    const int n = s->cfg.num_walkers / 2;
    REAL* pos = (REAL*)s->pos;
    REAL* lp = (REAL*)s->logp;
    REAL* cur_base = pos + (size_t)(color ? n : 0) * D;
    REAL* lp_base = lp + (color ? n : 0);
    uint32_t* acc_base = s->n_accept + (color ? n : 0);
    const REAL* other = pos + (size_t)(color ? 0 : n) * D;
    REAL* chain_base = chain_step ? chain_step + (size_t)(color ? n : 0) * D : NULL;
    const uint64_t threshold = (uint64_t)(0 - (uint64_t)n) % (uint64_t)n; /* pcg_extras bounded_rand */
    uint32_t accepted = 0;
    uint64_t ties = 0, redraws = 0;

    if (mode == SO_MODE_SEQUENTIAL) {
        for (int i = 0; i < n; ++i) {
            uint64_t r0;
            for (;;) {
                r0 = so_pcg64_next(eng);
                if (r0 >= threshold) break;
                ++redraws;
            }
            uint64_t r1 = so_pcg64_next(eng);
            uint64_t r2 = so_pcg64_next(eng);
            int a = SFX(update_walker)(s, cur_base + (size_t)i * D, lp_base + i, other, n, r0, r1, r2,
                                       chain_base ? chain_base + (size_t)i * D : NULL, &ties);
            acc_base[i] += (uint32_t)a;
            accepted += (uint32_t)a;
        }
    } else {
        /* counter-addressed: walker i owns draws 3*i .. 3*i+2 of this half-step */
        if (threads > n) threads = n;
#pragma omp parallel num_threads(threads) reduction(+ : accepted, ties, redraws)
        {
            int tid = 0, nt = 1;
#ifdef _OPENMP
            tid = omp_get_thread_num();
            nt = omp_get_num_threads();
#endif
            int lo = (int)((int64_t)n * tid / nt), hi = (int)((int64_t)n * (tid + 1) / nt);
            so_pcg64 g = *eng;
            so_pcg64_advance(&g, 0, 3ULL * (uint64_t)lo);
            for (int i = lo; i < hi; ++i) {
                uint64_t r0 = so_pcg64_next(&g);
                uint64_t r1 = so_pcg64_next(&g);
                uint64_t r2 = so_pcg64_next(&g);
                if (r0 < threshold) ++redraws; /* the reference would redraw: trajectories part here */
                int a = SFX(update_walker)(s, cur_base + (size_t)i * D, lp_base + i, other, n, r0, r1,
                                           r2, chain_base ? chain_base + (size_t)i * D : NULL, &ties);
                acc_base[i] += (uint32_t)a;
                accepted += (uint32_t)a;
            }
        }
        so_pcg64_advance(eng, 0, 3ULL * (uint64_t)n);
    }
    s->near_ties += ties;
    s->redraws += redraws;
    s->half_steps += 1;
    return accepted;
}

/* ---- next row f3: Mover::DifferentialEvolution ---------------------------------------------------------------------- */

/* One engine(n) of pcg64 (pcg_extras bounded_rand): draws below the threshold are thrown away and counted */
static uint64_t SFX(bounded)(so_pcg64* eng, uint64_t n, uint64_t threshold, uint64_t* extra)
{
    for (;;) {
        uint64_t r = so_pcg64_next(eng);
        if (r >= threshold) return r % n;
        ++*extra;
    }
}

/* One DifferentialEvolution::updateWalker (MCMCpp/Movers/DifferentialEvolution.h:80-112), drawing from `eng` in the
 * reference's order: ind1; ind2 until it differs from ind1; D uniform jitters; after the Calculator, the exponential.
 * The draw count is D + 3 plus the throw-aways, which are counted in *extra.  gamma and the jitter bounds are the
 * constructor's defaults: the samplers work on a copy of the user's mover, and the copy constructor
 * (DifferentialEvolution.h:65-69) re-initialises both, so overrideGamma/overrideRandBounds never reach a sampler. */
static int SFX(de_update_walker)(so_sampler* s, REAL* cur, REAL* cur_lp, const REAL* other, int n, so_pcg64* eng, REAL* row_out,
                                 uint64_t* extra, uint64_t* ties)
{
    const int D = s->cfg.num_params;
    REAL prop[D];
    const uint64_t threshold = (uint64_t)(0 - (uint64_t)n) % (uint64_t)n;
    const uint64_t ind1 = SFX(bounded)(eng, (uint64_t)n, threshold, extra);
    uint64_t ind2 = SFX(bounded)(eng, (uint64_t)n, threshold, extra);
    while (ind2 == ind1) {
        ++*extra;
        ind2 = SFX(bounded)(eng, (uint64_t)n, threshold, extra);
    }
    const REAL gamma = (REAL)(2.38 / sqrt((double)(2 * D))); /* DifferentialEvolution.h:57 */
    const REAL width = (REAL)2.0e-4, low = (REAL)-1.0e-4;   /* DifferentialEvolution.h:120-121 */
    const REAL* w1 = other + (size_t)ind1 * D;
    const REAL* w2 = other + (size_t)ind2 * D;
    for (int i = 0; i < D; ++i) {
        /* MultiSampler.h:66: lowEdge + realDist(engine) * width; realDist = uniform_real_distribution(0, 1): u * (1 - 0) + 0 */
        const REAL u = CANON(so_pcg64_next(eng)) * (REAL)1 + (REAL)0;
        prop[i] = cur[i] + gamma * (w1[i] - w2[i]) + (low + (u * width));
    }
    const REAL new_lp = SFX(calc_logp)(s->cfg.calc_id, D, (const REAL*)s->params, prop);
    const REAL u2 = CANON(so_pcg64_next(eng));
    const REAL neg_exp = -(-LOG((REAL)1 - u2) / (REAL)1);
    const REAL delta = new_lp - *cur_lp;
    const int accept = delta > neg_exp;
    {
        REAL margin = FABS(neg_exp - delta);
        REAL scale = FABS(neg_exp) + FABS(new_lp) + FABS(*cur_lp);
        if (SFX(near_tie)(margin, (REAL)TIE_EPS * scale)) ++*ties;
    }
    if (accept) {
        memcpy(cur, prop, sizeof(REAL) * (size_t)D);
        *cur_lp = new_lp;
    }
    if (row_out) memcpy(row_out, cur, sizeof(REAL) * (size_t)D);
    return accept;
}

/* One half of performStep with the DifferentialEvolution mover: sequential by nature of the stream (the next walker's
 * first draw follows this walker's last, and the count is data dependent) */
static uint32_t SFX(de_half_step)(so_sampler* s, int color, REAL* chain_step, so_pcg64* eng)
{
    const int D = s->cfg.num_params;
    const int n = s->cfg.num_walkers / 2;
    REAL* pos = (REAL*)s->pos;
    REAL* lp = (REAL*)s->logp;
    REAL* cur_base = pos + (size_t)(color ? n : 0) * D;
    REAL* lp_base = lp + (color ? n : 0);
    uint32_t* acc_base = s->n_accept + (color ? n : 0);
    const REAL* other = pos + (size_t)(color ? 0 : n) * D;
    REAL* chain_base = chain_step ? chain_step + (size_t)(color ? n : 0) * D : NULL;
    uint32_t accepted = 0;
    uint64_t extra = 0, ties = 0;
    for (int i = 0; i < n; ++i) {
        int a = SFX(de_update_walker)(s, cur_base + (size_t)i * D, lp_base + i, other, n, eng, chain_base ? chain_base + (size_t)i * D : NULL,
                                      &extra, &ties);
        acc_base[i] += (uint32_t)a;
        accepted += (uint32_t)a;
    }
    s->redraws += extra;
    s->near_ties += ties;
    s->half_steps += 1;
    return accepted;
}

/* walkers [begin, begin+count) of one colour, counter-addressed; does not advance half_steps */
static uint32_t SFX(half_step_shard)(so_sampler* s, int color, int begin, int count)
{
    const int D = s->cfg.num_params;
    const int n = s->cfg.num_walkers / 2;
    REAL* pos = (REAL*)s->pos;
    REAL* lp = (REAL*)s->logp;
    REAL* cur_base = pos + (size_t)(color ? n : 0) * D;
    REAL* lp_base = lp + (color ? n : 0);
    uint32_t* acc_base = s->n_accept + (color ? n : 0);
    const REAL* other = pos + (size_t)(color ? 0 : n) * D;
    const uint64_t threshold = (uint64_t)(0 - (uint64_t)n) % (uint64_t)n;
    so_pcg64 g = s->eng0;
    {
        u128 d = (u128)3u * (u128)(uint64_t)n * (u128)s->half_steps + (u128)3u * (u128)(uint64_t)begin;
        so_pcg64_advance(&g, (uint64_t)(d >> 64), (uint64_t)d);
    }
    uint32_t accepted = 0;
    uint64_t ties = 0;
    for (int i = begin; i < begin + count; ++i) {
        uint64_t r0 = so_pcg64_next(&g), r1 = so_pcg64_next(&g), r2 = so_pcg64_next(&g);
        if (r0 < threshold) s->redraws += 1;
        int a = SFX(update_walker)(s, cur_base + (size_t)i * D, lp_base + i, other, n, r0, r1, r2, NULL, &ties);
        acc_base[i] += (uint32_t)a;
        accepted += (uint32_t)a;
    }
    s->near_ties += ties;
    return accepted;
}

/* EnsembleSampler::runMCMC (EnsembleSampler.h:284-310): per stored step, interval-1 unsaved
 * ensemble steps then one saved step. */
static int SFX(run)(so_sampler* s, int64_t n_saved, int32_t interval, REAL* chain_out,
                    uint32_t* accepted_per_step, int mode, int threads)
{
    const size_t W = (size_t)s->cfg.num_walkers, D = (size_t)s->cfg.num_params;
    const uint64_t n = (uint64_t)(W / 2);
    const int de = s->cfg.mover == SO_MOVER_DIFFERENTIAL_EVOLUTION;
    /* engine at the first draw of half-step `half_steps` (3 draws per stretch update, D + 3 per differential-evolution
     * update, n updates per half, plus every draw thrown away so far) */
    so_pcg64 eng = s->eng0;
    {
        u128 d = (u128)(de ? (uint64_t)D + 3u : 3u) * (u128)n * (u128)s->half_steps + (u128)s->redraws;
        so_pcg64_advance(&eng, (uint64_t)(d >> 64), (uint64_t)d);
    }
    int64_t step = 0;
    for (int64_t k = 0; k < n_saved; ++k) {
        for (int32_t j = 0; j < interval; ++j, ++step) {
            int save = (j == interval - 1) && chain_out;
            REAL* row = save ? chain_out + (size_t)k * W * D : NULL;
            uint32_t a = de ? SFX(de_half_step)(s, 0, row, &eng) : SFX(half_step)(s, 0, row, mode, threads, &eng);
            a += de ? SFX(de_half_step)(s, 1, row, &eng) : SFX(half_step)(s, 1, row, mode, threads, &eng);
            if (accepted_per_step) accepted_per_step[step] = a;
        }
    }
    return 0;
}

/* Analysis::CovarianceMatrix::calculateCovar + finalizeMatrix (MCMCpp/Analysis/CovarianceMatrix.h:154-224): Kahan sums
 * of x_i and x_i*x_j over every `slice`-th stored step and all walkers, in the reference's order (step, walker,
 * i, j <= i), then cov = E[xy] - E[x]E[y] and the correlation matrix (rows, then columns, divided by the square
 * roots of the variances).  `steps` is [n_steps][W][D]; cov / corr are [D][D]; mean (may be NULL) is [D]. */
static void SFX(chain_covariance)(const REAL* steps, int64_t n_steps, int W, int D, int slice, REAL* mean, REAL* cov, REAL* corr)
{
    const size_t DD = (size_t)D * (size_t)D;
    REAL* prod = (REAL*)calloc(DD, sizeof(REAL));
    REAL* prod_c = (REAL*)calloc(DD, sizeof(REAL));
    REAL* avg = (REAL*)calloc((size_t)D, sizeof(REAL));
    REAL* avg_c = (REAL*)calloc((size_t)D, sizeof(REAL));
    int64_t used = 0;
    for (int64_t st = 0; st < n_steps; ++st) {
        if (st % slice != 0) continue;
        for (int w = 0; w < W; ++w) {
            const REAL* pt = steps + ((size_t)st * (size_t)W + (size_t)w) * (size_t)D;
            for (int i = 0; i < D; ++i) {
                { /* addAverage, CovarianceMatrix.h:251-257 */
                    REAL y = pt[i] - avg_c[i];
                    REAL t = avg[i] + y;
                    avg_c[i] = (t - avg[i]) - y;
                    avg[i] = t;
                }
                for (int j = 0; j <= i; ++j) { /* addProduct, CovarianceMatrix.h:229-247: both orders hold the same sum */
                    const REAL val = pt[i] * pt[j];
                    size_t o = (size_t)i * D + j;
                    REAL y = val - prod_c[o];
                    REAL t = prod[o] + y;
                    prod_c[o] = (t - prod[o]) - y;
                    prod[o] = t;
                    if (i != j) {
                        o = (size_t)j * D + i;
                        y = val - prod_c[o];
                        t = prod[o] + y;
                        prod_c[o] = (t - prod[o]) - y;
                        prod[o] = t;
                    }
                }
            }
        }
        ++used;
    }
    /* the reference forms the count in int arithmetic first (numUsedSteps*wCount, CovarianceMatrix.h:181) */
    const REAL count = (REAL)(int)(used * (int64_t)W);
    for (int i = 0; i < D; ++i) avg[i] /= count;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
            REAL t = (prod[(size_t)i * D + j] / count) - (avg[i] * avg[j]);
            cov[(size_t)i * D + j] = t;
            cov[(size_t)j * D + i] = t;
        }
    for (int i = 0; i < D; ++i) {
        REAL sv = SQRT(cov[(size_t)i * D + i]);
        for (int j = 0; j < D; ++j) corr[(size_t)i * D + j] = cov[(size_t)i * D + j] / sv;
    }
    for (int j = 0; j < D; ++j) {
        REAL sv = SQRT(cov[(size_t)j * D + j]);
        for (int i = 0; i < D; ++i) corr[(size_t)i * D + j] /= sv;
    }
    if (mean) memcpy(mean, avg, sizeof(REAL) * (size_t)D);
    free(prod);
    free(prod_c);
    free(avg);
    free(avg_c);
}

/* ---- Analysis::Detail::AutoCov and Analysis::AutoCorrCalc (next row f2) -------------------------------------------- */

static unsigned SFX(bit_reverse)(unsigned x, int lg)
{ /* Detail/AutoCov.h:255-266 */
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    x = (x >> 16) | (x << 16);
    return x >> (32 - lg);
}

/* Detail::AutoCov::calcNormAutoCov (Detail/AutoCov.h:146-155): the series minus its average, zero-extended to the next
 * power of two >= n (NOT to 2n: the autocovariance is circular), iterative radix-2 Cooley-Tukey forward transform,
 * |.|^2, inverse transform without the 1/N factor, everything divided by element 0.  Complex products are
 * (ac - bd, ad + bc) with individually rounded terms, as the compiler's complex multiplication yields for finite
 * values.  work: 2 * fft complex scratch; tw: fft/2 (cos, sin) pairs of 2 pi i / fft.  chain[0..n) in, autocov out. */
static int SFX(fft_log2)(int n) { return (int)ceil(log2((double)n)); } /* AutoCov.h:318-322 */
static void SFX(fft_twiddles)(int lg, REAL* tw)
{ /* AutoCov.h:304-315; TwoPi from the rational constant of AutoCov.h:29-30,135 */
    const int fft = 1 << lg;
    const REAL two_pi = (REAL)2 * ((REAL)3141592653589793239ULL / (REAL)1000000000000000000ULL);
    for (int i = 0; i < fft / 2; ++i) {
        REAL angle = two_pi * (REAL)i / (REAL)fft;
        /* the reference writes std::cos(angle), std::sin(angle); g++ -O2 (its toolchain, and this oracle's) folds the pair
         * into ONE sincos call, whose results are not bit-identical to separate cos and sin calls for every angle
         * (entry 1955 of the 4096-point table differs).  Stated explicitly so that no compiler choice changes it. */
        SINCOS(angle, &tw[2 * i + 1], &tw[2 * i]);
    }
}
static void SFX(fft_pass)(REAL* a /* fft complex, bit-reversed input */, int lg, const REAL* tw, REAL sign)
{ /* AutoCov.h:166-185 (inverse, sign +1) and 197-216 (forward, sign -1) */
    const int fft = 1 << lg;
    for (int s = 1; s <= lg; ++s) {
        const int m1 = 1 << s, m2 = m1 >> 1, stride = fft >> s;
        for (int k = 0; k < fft; k += m1) {
            int ti = 0;
            for (int j = 0; j < m2; ++j) {
                const REAL wr = tw[2 * ti], wi = sign * tw[2 * ti + 1];
                const REAL br = a[2 * (k + j + m2)], bi = a[2 * (k + j + m2) + 1];
                const REAL t1r = wr * br - wi * bi, t1i = wr * bi + wi * br;
                const REAL t2r = a[2 * (k + j)], t2i = a[2 * (k + j) + 1];
                a[2 * (k + j)] = t2r + t1r;
                a[2 * (k + j) + 1] = t2i + t1i;
                a[2 * (k + j + m2)] = t2r - t1r;
                a[2 * (k + j + m2) + 1] = t2i - t1i;
                ti += stride;
            }
        }
    }
}
static void SFX(norm_autocov)(REAL* chain, REAL avg, int n, int lg, const REAL* tw, REAL* work)
{
    const int fft = 1 << lg;
    REAL* first = work;
    REAL* second = work + 2 * (size_t)fft;
    for (int i = 0; i < n; ++i) { /* AutoCov.h:241-252 */
        const unsigned r = SFX(bit_reverse)((unsigned)i, lg);
        first[2 * r] = chain[i] - avg;
        first[2 * r + 1] = (REAL)0;
    }
    for (int i = n; i < fft; ++i) {
        const unsigned r = SFX(bit_reverse)((unsigned)i, lg);
        first[2 * r] = (REAL)0;
        first[2 * r + 1] = (REAL)0;
    }
    SFX(fft_pass)(first, lg, tw, (REAL)-1);
    for (int i = 0; i < fft; ++i) { /* AutoCov.h:187-195 */
        const unsigned r = SFX(bit_reverse)((unsigned)i, lg);
        second[2 * r] = first[2 * i] * first[2 * i] + first[2 * i + 1] * first[2 * i + 1];
        second[2 * r + 1] = (REAL)0;
    }
    SFX(fft_pass)(second, lg, tw, (REAL)1);
    const REAL norm = second[0];
    for (int i = 0; i < n; ++i) chain[i] = second[2 * i] / norm; /* AutoCov.h:157-163 */
}

/* Analysis::AutoCorrCalc::calcAutoCorrTimes with every walker used (AutoCorrCalc.h:151-207,239-264): per walker and
 * parameter the Kahan average over the n steps; per parameter the normalised autocovariance functions of all walkers
 * summed (with the reference's own compensation formula) and divided by W; then the windowed sum.
 * emulate_defect != 0 restates the reference to the letter: transferWalker (AutoCorrCalc.h:239-245) ADDS each
 * series onto what the scratch array holds -- the previous walker's autocovariance function (zeros before the
 * first, assuming fresh memory) -- instead of overwriting it.  With 0 the series replaces the scratch content, which
 * is what the function is documented to compute; that is what the device implementation is held to. */
static void SFX(autocorr_times)(const REAL* steps, int n, int W, int D, int window_scaling, int emulate_defect, REAL* out, REAL* functions)
{
    const int lg = SFX(fft_log2)(n), fft = 1 << lg;
    REAL* tw = (REAL*)malloc(sizeof(REAL) * (size_t)fft);
    REAL* work = (REAL*)malloc(sizeof(REAL) * 4 * (size_t)fft);
    REAL* acov = (REAL*)calloc((size_t)n, sizeof(REAL));
    REAL* sum = (REAL*)malloc(sizeof(REAL) * (size_t)n);
    REAL* comp = (REAL*)malloc(sizeof(REAL) * (size_t)n);
    REAL* avg = (REAL*)calloc((size_t)W * D, sizeof(REAL));
    REAL* avg_c = (REAL*)calloc((size_t)W * D, sizeof(REAL));
    SFX(fft_twiddles)(lg, tw);
    for (int t = 0; t < n; ++t) /* calculateChainAverages, AutoCorrCalc.h:248-276 */
        for (int j = 0; j < W * D; ++j) {
            REAL value = steps[(size_t)t * W * D + j] - avg_c[j];
            REAL temp = avg[j] + value;
            avg_c[j] = (temp - avg[j]) - value;
            avg[j] = temp;
        }
    for (int j = 0; j < W * D; ++j) avg[j] /= (REAL)n;
    for (int p = 0; p < D; ++p) { /* sampleParamAutoCorrTimes, AutoCorrCalc.h:170-207 */
        for (int i = 0; i < n; ++i) sum[i] = comp[i] = (REAL)0;
        for (int w = 0; w < W; ++w) {
            for (int t = 0; t < n; ++t) {
                const REAL x = steps[((size_t)t * W + w) * D + p];
                acov[t] = emulate_defect ? x + acov[t] : x;
            }
            SFX(norm_autocov)(acov, avg[(size_t)w * D + p], n, lg, tw, work);
            for (int i = 0; i < n; ++i) { /* averageAutocovarianceFunctions, AutoCorrCalc.h:209-221 */
                REAL value = acov[i] + comp[i];
                REAL temp = sum[i] + value;
                comp[i] = (temp - sum[i]) - value;
                sum[i] = temp;
            }
        }
        for (int i = 0; i < n; ++i) sum[i] /= (REAL)W;
        if (functions) memcpy(functions + (size_t)p * n, sum, sizeof(REAL) * (size_t)n);
        REAL acs = -sum[0], c = (REAL)0, result = (REAL)0;
        const REAL factor = (REAL)window_scaling;
        int converged = 0;
        for (int i = 0; i < n; ++i) {
            REAL value = ((REAL)2 * sum[i]) - c;
            REAL temp = acs + value;
            c = (temp - acs) - value;
            acs = temp;
            if ((REAL)i > factor * acs) {
                result = acs;
                converged = 1;
                break;
            }
        }
        out[p] = converged ? result : -acs;
    }
    free(tw); free(work); free(acov); free(sum); free(comp); free(avg); free(avg_c);
}
