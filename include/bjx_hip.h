/*
 * bjx_hip.h -- C ABI of libbjxhip.so, the MI355X (gfx950) engine behind
 * blackjax_amd.hmc / .nuts / .window_adaptation.
 *
 * The reference (blackjax-devs/blackjax) has no FFI: its hot path is a Python
 * protocol (blackjax/base.py:88-113, SamplingAlgorithm(init, step)).  This header
 * is the boundary a maintainer would bind (ctypes stub in INTEGRATION.md); every
 * entry point cites the reference function(s) whose arithmetic it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every function returns 0 on success, non-zero on failure;
 *     bjx_last_error() returns a thread-local message for the last failure.
 *   - all array pointers are DEVICE pointers owned by the caller; nothing is
 *     allocated inside a call; calls are asynchronous on `stream` (a hipStream_t
 *     passed as void*), re-entrant, no global mutable state.
 *   - chain-major row layout: an (N, D) array is N rows of D contiguous fp32.
 *   - `key` arguments are threefry keys passed BY VALUE as two uint32 words
 *     (jax.random key data); per-chain keys are derived in-kernel so sharded runs need
 *     no exchange.  Two layouts, selected by `step_fold`:
 *       step_fold <  0  "step-major":  k_i = split(key, .)[chain_offset+i]
 *                       (key = this step's key; vmap inside the step)
 *       step_fold >= 0  "chain-major": k_i = split(split(key, .)[chain_offset+i], .)[step_fold]
 *                       (key = the run key, step_fold = t; vmap over whole per-chain loops,
 *                       e.g. a vmapped window_adaptation(...).run)
 *   - `eps` (step size): if `eps_per_chain` != NULL it is a device (N,) array,
 *     otherwise the scalar `eps` is used for every chain.
 *   - `imm` (diagonal inverse mass matrix): row stride `imm_stride` = 0 for one
 *     shared (D,) vector, = D for a per-chain (N, D) array.
 */
#ifndef BJX_HIP_H
#define BJX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_ABI_VERSION 7 /* 2: bjx_nuts_t gained int_kick / int_drift (round 3); 3: bjx_nuts_async_t gained int_stages /
                             int_mid_kick / int_mid_drift, bjx_rng_key_probe added (round 4); 4: bjx_nuts_async_t gained
                             gemm_pc .. gemm_cap (round 4); 5 (round 5): same entry points and layouts -- bjx_nuts_async_tick now
                             has ONE kernel per shape and reads no environment switch (an engine-resident target is ticked
                             ticks_per_launch >= 1 times per launch whatever the batch size; run->end_list / end_count are
                             only used in GEMM mode), multi-stage integrators tick free for rows of up to 1 024 floats, and the
                             shared-dense entry points REFUSE whole 128 x 128 tiles on buffers that are not 16-byte aligned
                             instead of reading imm transposed; 6 (round 5): bjx_nuts_spec_t and bjx_nuts_spec_enter / _integrate /
                             _book added (two-stream speculative tail of a free-running run), nothing else changed; 7 (round 6):
                             bjx_log1p_device_check added; the NUTS `is` table gained the slot BJX_NUTS_I_STAGE
                             (BJX_NUTS_NI 17 -> 18: multi-stage integrators on the general free-running tick kernel) */

const char* bjx_last_error(void);
int bjx_abi_version(void);

/* jax.random.split(key, n)[offset : offset+n] on the host (no device work).
 * Replaces: jax.random.split at blackjax/util.py:203, adaptation/staged_adaptation.py:868.
 * out: host uint32[n][2]. */
int bjx_keys_split(uint32_t key0, uint32_t key1, int64_t n, int64_t offset, uint32_t* out);

/* Debug/parity probes of the in-kernel RNG (device): z[i][j] = jax.random.normal(
 * split(key, .)[chain_offset+i] , (D,))[j]  and  u[i] = jax.random.uniform(same key, ()).
 * Replaces: jax.random.normal at blackjax/util.py:90; jax.random.uniform inside bernoulli
 * at blackjax/mcmc/proposal.py:226. */
int bjx_rng_normal(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                   int64_t N, int64_t D, float* z_out);
int bjx_rng_uniform(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                    int64_t N, float* u_out);
/* The same device functions with the key used AS IS (no per-chain child key):
 *   z_out[j] = jax.random.normal(key, (D,))[j] ; u_out[0] = jax.random.uniform(key, ()) (may be NULL) ;
 *   children_out[i][0..1] = jax.random.split(key, n_children)[i]  (device uint32[n_children][2]).
 * The probe the jax.random values printed in JAX's documentation are held against (tests/golden/
 * reference_kats.json "jax_docs_streams").  Replaces: jax.random.normal / uniform / split as used at
 * blackjax/util.py:90, mcmc/proposal.py:226, mcmc/hmc.py:299. */
int bjx_rng_key_probe(void* stream, uint32_t key0, uint32_t key1, int64_t D, float* z_out, float* u_out,
                      int64_t n_children, uint32_t* children_out);

/* Device self-check of the correctly-rounded fp32 -log1p inside jax.random.normal's erf_inv (csrc/bjx_log1p.h): every
 * stride-th fp32 t in (-1, 0] through the product's function against the device library's fp64 log1p rounded once.
 * counts_out: device uint64[4] = {inputs checked, results that differ, inputs resolved by the slow table, bit
 * pattern of the first differing input}.  stride 1 = exhaustive (1 065 353 217 inputs, ~0.1 s).
 * Checks the arithmetic behind: jax.random.normal as used at blackjax/util.py:88-91. */
int bjx_log1p_device_check(void* stream, uint32_t stride, unsigned long long* counts_out);

/* Momentum draw for a diagonal metric + initial kinetic energy.
 *   k_i = split(key, .)[chain_offset+i]; km = split(k_i, 2)[0]
 *   p0[i] = (1/sqrt(imm)) * normal(km, (D,)) ;  ke0[i] = 0.5 * dot(imm*p0[i], p0[i])
 * Replaces: blackjax/mcmc/hmc.py:299,302 ; metrics.py:260-261,263-270,704-709 ; util.py:66-91. */
int bjx_hmc_momentum_diag(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                          int64_t step_fold, int64_t N, int64_t D, const float* imm, int64_t imm_stride,
                          float* p_out, float* ke_out);

/* bjx_hmc_momentum_diag followed by bjx_leapfrog_diag(n_kicks = 1) in ONE launch (same arithmetic,
 * same results): additionally  p_half = p0 + (eps_i / 2) g0 ;  q1 = q0 + eps_i * (imm_i * p_half)
 * (integrators.py:104-150, first half of the trajectory's first velocity-Verlet step).  The momentum
 * draw is bound by its per-element RNG arithmetic, so the first kick + drift ride along.          */
int bjx_hmc_momentum_kick_diag(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                               int64_t step_fold, int64_t N, int64_t D, const float* imm, int64_t imm_stride,
                               float eps, const float* eps_per_chain, const float* q0, const float* g0,
                               float* p_out, float* ke_out, float* q1_out, float* p_half_out);

/* Fused velocity-Verlet "kick(s) + drift" for a diagonal metric:
 *   n_kicks = 1:  p = p + (eps/2) g                       (first step of a trajectory)
 *   n_kicks = 2:  p = (p + (eps/2) g) + (eps/2) g         (closing half kick of the previous
 *                                                          step + opening half kick of this one;
 *                                                          two separately rounded fmas)
 *   v = imm * p ;  q = q + eps * v
 * reads p_in, g, q_in ; writes p_out, q_out (may alias the inputs).
 * Replaces: blackjax/mcmc/integrators.py:104-150 (one_step), 191-205, 226-243 with
 * coefficients [0.5, 1.0, 0.5] (321-322), driven by trajectory.py:155-165. */
int bjx_leapfrog_diag(void* stream, int64_t N, int64_t D, int n_kicks, float eps,
                      const float* eps_per_chain, const float* imm, int64_t imm_stride,
                      const float* q_in, const float* p_in, const float* g, float* q_out,
                      float* p_out);

/* Same as bjx_leapfrog_diag with a per-chain trajectory length (dynamic HMC, SURVEY.md section 8f
 * row 2): chain i is advanced only while step_idx < n_steps[i] (n_steps: device (N,) int32);
 * otherwise its (q, p) is left untouched (copied through when the launch is out of place).
 * Replaces: the per-chain `num_integration_steps` of blackjax/mcmc/dynamic_hmc.py:85-118 under vmap. */
int bjx_leapfrog_diag_masked(void* stream, int64_t N, int64_t D, int n_kicks, float eps,
                             const float* eps_per_chain, const float* imm, int64_t imm_stride,
                             const float* q_in, const float* p_in, const float* g, float* q_out,
                             float* p_out, const int32_t* n_steps, int32_t step_idx);

/* General palindromic integrators: coefficients
 * [b1, a1, b2, a2, ..., b1] of generalized_two_stage_integrator (blackjax/mcmc/integrators.py:
 * 104-150; mclachlan / yoshida / omelyan 335-369).  One launch per position update:
 *   p = p + (eps*kick_a) g  [ ; p = p + (eps*kick_b) g  if n_kicks == 2 ]
 *   q = q + (eps*drift) * (imm * p)
 * `eps*coef` is an fp32 product like the reference's `step_size * coef`.  Velocity Verlet is
 * (kick_a, kick_b, drift) = (0.5, 0.5, 1.0), i.e. bjx_leapfrog_diag.  n_steps/step_idx as in
 * bjx_leapfrog_diag_masked (NULL = every chain advances). */
int bjx_leapfrog_diag_coef(void* stream, int64_t N, int64_t D, int n_kicks, float kick_a,
                           float kick_b, float drift, float eps, const float* eps_per_chain,
                           const float* imm, int64_t imm_stride, const float* q_in,
                           const float* p_in, const float* g, float* q_out, float* p_out,
                           const int32_t* n_steps, int32_t step_idx);

/* bjx_hmc_finish_diag with the closing kick p1 = p + (eps*kick_coef) g1, kick_coef = last
 * coefficient of the palindromic integrator (0.5 for velocity Verlet). */
int bjx_hmc_finish_diag_coef(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                             int64_t step_fold, int64_t N, int64_t D, float kick_coef, float eps,
                             const float* eps_per_chain, const float* imm, int64_t imm_stride,
                             float divergence_threshold, const float* q0, const float* logp0,
                             const float* g0, const float* ke0, const float* q1, const float* logp1,
                             const float* g1, const float* p, float* p_end_out, float* q_out,
                             float* logp_out, float* g_out, float* acceptance_rate_out,
                             uint8_t* is_accepted_out, uint8_t* is_divergent_out, float* energy_out);

/* Per-chain key utilities on the device (keys: (N, 2) uint32 jax.random key data).
 *   bjx_keys_child:   keys_out[i] = split(keys_in[i], .)[child]   (default next_random_arg_fn of
 *                     dynamic_hmc.py:69: `lambda key: jax.random.split(key)[1]`)
 *   bjx_keys_randint: out[i] = jax.random.randint(keys[i], (), minval, maxval) as int32 (default
 *                     integration_steps_fn of dynamic_hmc.py:70: randint(key, (), 1, 10)).
 * jax.random.randint is restated from jax/_src/random.py::_randint (two 32-bit draws from
 * split(key, 2), offset = ((hi % span) * (2^32 % span) + lo % span) % span). */
int bjx_keys_child(void* stream, int64_t N, const uint32_t* keys_in, uint32_t child,
                   uint32_t* keys_out);
int bjx_keys_randint(void* stream, int64_t N, const uint32_t* keys, int32_t minval, int32_t maxval,
                     int32_t* out);

/* Closing half kick + flip + energies + Metropolis accept + state select (diag metric).
 *   p1 = p + (eps/2) g1 ; p_end = -p1 ; ke1 = 0.5 dot(imm*p1, p1)
 *   H0 = -logp0 + ke0 ; H1 = -logp1 + ke1 ; delta = H0 - H1 (NaN -> -inf)
 *   is_divergent = -delta > divergence_threshold ; p_acc = min(1, exp(delta))
 *   ki = split(split(key,.)[chain_offset+i], 2)[1] ; accept = uniform(ki) < p_acc
 *   (q,logp,g)_out = accept ? (q1,logp1,g1) : (q0,logp0,g0)
 * p_end_out may be NULL (HMCInfo.proposal.momentum not wanted) or alias p.
 * Replaces: blackjax/mcmc/hmc.py:95-112,153-176 ; trajectory.py:730-750 ;
 * proposal.py:45-48,214-235. */
int bjx_hmc_finish_diag(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                        int64_t step_fold, int64_t N, int64_t D, float eps, const float* eps_per_chain,
                        const float* imm, int64_t imm_stride, float divergence_threshold,
                        const float* q0, const float* logp0, const float* g0, const float* ke0,
                        const float* q1, const float* logp1, const float* g1, const float* p,
                        float* p_end_out, float* q_out, float* logp_out, float* g_out,
                        float* acceptance_rate_out, uint8_t* is_accepted_out,
                        uint8_t* is_divergent_out, float* energy_out);

/* ---- multinomial HMC (blackjax.mhmc) ----------------------------
 * One step of static_progressive_integration fused with the opening half of the next leapfrog.
 * On entry p holds the momentum after the OPENING half kick of leapfrog `step` and (q, g,
 * logp_new) the new position and the callable's outputs there.  The kernel applies the closing
 * half kick, forms the proposal weight w = H0 - H (NaN -> -inf), any_divergent |= -w > threshold,
 * draws u = uniform(fold_in(key_integrator, step)), accepts the new state into the reservoir
 * (prop_*) with probability expit(w - weight), updates weight and sum_log_p_accept by logaddexp,
 * and, if do_next, performs the opening half kick + drift of leapfrog step+1 in place on (q, p).
 * weight / sum_log_p_accept: (N,) initialised to 0 / -inf; ever_accepted / any_divergent: (N,)
 * uint8 initialised to 0.  H0 = -logp0 + ke0.
 * Replaces: blackjax/mcmc/hmc.py:181-248 ; trajectory.py:170-232 ; proposal.py:51-105,118-143. */
int bjx_mhmc_step_diag(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                       int64_t step_fold, int64_t N, int64_t D, int64_t step, int do_next, float eps,
                       const float* eps_per_chain, const float* imm, int64_t imm_stride,
                       float divergence_threshold, const float* logp0, const float* ke0, float* q,
                       float* p, const float* g, const float* logp_new, float* weight,
                       float* sum_log_p_accept, uint8_t* any_divergent, uint8_t* ever_accepted,
                       float* prop_q, float* prop_p, float* prop_g, float* prop_logp,
                       float* prop_energy);

/* End of a multinomial-HMC transition: chains whose reservoir never replaced the initial state get
 * (q0, p0, g0, logp0, H0) copied into prop_*; acceptance_rate = exp(sum_log_p_accept) / L
 * (hmc.py:234).  prop_(q, logp, g) is the new chain state. */
int bjx_mhmc_finish(void* stream, int64_t N, int64_t D, int64_t num_integration_steps,
                    const float* q0, const float* p0, const float* g0, const float* logp0,
                    const float* ke0, const uint8_t* ever_accepted, const float* sum_log_p_accept,
                    float* prop_q, float* prop_p, float* prop_g, float* prop_logp, float* prop_energy,
                    float* acceptance_rate_out);

/* The same two entry points with one trajectory length PER CHAIN (blackjax.dmhmc =
 * dynamic_hmc.build_kernel(build_proposal=multinomial_hmc_proposal), blackjax/__init__.py:155-163;
 * dynamic_hmc.py:85-118 under vmap): chain i takes part in step `step` only while step < n_steps[i]
 * (device (N,) int32), its last step opens no further leapfrog, and its acceptance rate is
 * exp(sum_log_p_accept[i]) / n_steps[i]. */
int bjx_mhmc_step_diag_masked(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                              int64_t step_fold, int64_t N, int64_t D, int64_t step, int do_next, float eps,
                              const float* eps_per_chain, const float* imm, int64_t imm_stride,
                              float divergence_threshold, const float* logp0, const float* ke0, float* q,
                              float* p, const float* g, const float* logp_new, float* weight,
                              float* sum_log_p_accept, uint8_t* any_divergent, uint8_t* ever_accepted,
                              float* prop_q, float* prop_p, float* prop_g, float* prop_logp,
                              float* prop_energy, const int32_t* n_steps);
/* bjx_mhmc_step_diag[_masked] for any palindromic integrator [b_1, a_1, ..., b_1] (blackjax.mhmc /
 * dmhmc with integrator=mclachlan / yoshida / omelyan; blackjax/mcmc/integrators.py:335-369 through
 * trajectory.py:170-232): the closing kick of the step and -- with do_next -- the opening kick of the
 * next one are (eps * kick_coef) g, the drift that follows is (eps * drift_coef) imm p; the stages in
 * between (b_2, a_2 ...) are bjx_leapfrog_diag_coef launches with n_kicks = 1.  n_steps may be NULL
 * (every chain advances).  (0.5, 1.0) reproduces bjx_mhmc_step_diag bit for bit. */
int bjx_mhmc_step_diag_coef(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                            int64_t step_fold, int64_t N, int64_t D, int64_t step, int do_next, float eps,
                            const float* eps_per_chain, const float* imm, int64_t imm_stride,
                            float divergence_threshold, const float* logp0, const float* ke0, float* q,
                            float* p, const float* g, const float* logp_new, float* weight,
                            float* sum_log_p_accept, uint8_t* any_divergent, uint8_t* ever_accepted,
                            float* prop_q, float* prop_p, float* prop_g, float* prop_logp,
                            float* prop_energy, const int32_t* n_steps, float kick_coef, float drift_coef);

int bjx_mhmc_finish_masked(void* stream, int64_t N, int64_t D, const int32_t* n_steps, const float* q0,
                           const float* p0, const float* g0, const float* logp0, const float* ke0,
                           const uint8_t* ever_accepted, const float* sum_log_p_accept, float* prop_q,
                           float* prop_p, float* prop_g, float* prop_logp, float* prop_energy,
                           float* acceptance_rate_out);

/* ---- dense Gaussian-Euclidean metric (one (D, D) inverse mass matrix shared by all chains) ----
 * fp32 MFMA GEMMs (v_mfma_f32_32x32x2_f32, exact fp32 fma chains: "precision=highest",
 * blackjax/util.py:23-61).  All matrices row-major.
 *
 * C = A @ B with A (N, D), B (D, D): the building block, exported for parity tests. */
int bjx_dense_matmul(void* stream, int64_t N, int64_t D, const float* A, const float* B, float* C);

/* V = P imm^T -- v_r = imm p_r for every row, the matrix read AS STORED (v[i] = sum_k imm[i][k] p[k],
 * blackjax/mcmc/metrics.py:263-304 `linear_map`) -- given imm AND its transpose imm_t (both (D, D) row-major).
 * bjx_dense_apply_imm with three differences: few rows (N D <= BJX_DENSE_SKINNY_MAX, default 2^19) run on a
 * latency-oriented kernel (a few microseconds instead of 18-28), ragged shapes use imm_t on the general kernel --
 * so a matrix that is symmetric only up to rounding (a Welford covariance) gives the same product at every batch
 * size -- and whole aligned tiles run on the kernel bjx_dense_apply_imm uses.  One ascending-k fp32 fma chain per
 * output element in the k order of the MFMA kernels everywhere: identical results.  (round 4) */
int bjx_dense_apply_imm_t(void* stream, int64_t N, int64_t D, const float* P, const float* imm, const float* imm_t,
                          float* V);

/* C = A B like bjx_dense_matmul, given B AND its transpose Bt (both (D, D) row-major): whole 128-row / 128-column
 * tiles of 16-byte aligned buffers run on the kernel that reads its matrix as stored (the one bjx_dense_apply_imm uses
 * for a symmetric matrix, faster), few rows (N D <= BJX_DENSE_SKINNY_MAX) on the latency-oriented kernel of
 * bjx_dense_apply_imm_t, anything else on bjx_dense_matmul's kernel.  Same ascending-k fp32 fma chain per
 * output element either way: identical results.  (round 4) */
int bjx_dense_matmul_bt(void* stream, int64_t N, int64_t D, const float* A, const float* B, const float* Bt, float* C);

/* V = P @ imm^T for N rows: v_i = imm p_i (linear_map(inverse_mass_matrix, p), util.py:58-61;
 * metrics.py:263-304) on the fp32 MFMA GEMM, imm read as the reference stores it (row n = output n).
 * Complete 128 x 128 tiles take the k-contiguous "TN" kernel, which reads imm[i][k]; ragged shapes run on the general
 * kernel, which walks imm[k][i] -- the same product for an EXACTLY symmetric matrix only.  For a matrix that is
 * symmetric up to rounding (a dense Welford estimate) use bjx_dense_apply_imm_t, which takes the transposed copy too
 * and reads the matrix as stored at every shape (what dense-metric NUTS and the Python layer do since round 4; the
 * fused entry points -- bjx_leapfrog_dense, bjx_hmc_finish_dense, ... -- follow the same rule, so their callers pass
 * the transposed copy as `imm` for ragged shapes: blackjax_amd/dense.py::_imm_ptr). */
int bjx_dense_apply_imm(void* stream, int64_t N, int64_t D, const float* P, const float* imm, float* V);

/* Momentum draw: z = normal(km, (D,)) ; p = L^{-T} z = z @ mass_sqrt_t with mass_sqrt_t = L^{-1}
 * (L = cholesky(imm, lower)) ; ke = 0.5 dot(imm @ p, p).  z_work, v_work: (N, D) scratch.
 * Replaces: blackjax/mcmc/hmc.py:299,302 ; metrics.py:260-261,263-270,711-715 ; util.py:58-61,89-91. */
int bjx_hmc_momentum_dense(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                           int64_t step_fold, int64_t N, int64_t D, const float* mass_sqrt_t,
                           const float* imm, float* z_work, float* v_work, float* p_out,
                           float* ke_out);

/* Fused kick(s) + drift with a dense metric: p' = kick(p, g) [GEMM A-operand prologue, written to
 * p_out] ; v = imm @ p' [MFMA] ; q_out = q_in + eps v [epilogue].  p_out must not alias p_in;
 * q_out may alias q_in.  Replaces: blackjax/mcmc/integrators.py:104-150 with util.py:58-61. */
int bjx_leapfrog_dense(void* stream, int64_t N, int64_t D, int n_kicks, float eps,
                       const float* eps_per_chain, const float* imm, const float* q_in,
                       const float* p_in, const float* g, float* q_out, float* p_out);

/* Dense-metric counterparts of bjx_leapfrog_diag_coef / bjx_leapfrog_diag_masked,
 * bjx_hmc_finish_diag_coef and bjx_mhmc_step_diag (the reference's
 * multinomial_hmc_proposal, dynamic_hmc and palindromic integrators work with any metric,
 * blackjax/mcmc/hmc.py:181-248, dynamic_hmc.py:65-126, integrators.py:335-369).
 * matrix_stride < 0: ONE (D, D) matrix shared by all chains, applied on the fp32 MFMA GEMM
 * (p_out must not alias p_in); matrix_stride = 0 or D*D: the fp64-accumulated matrix-vector kernels
 * (shared matrix / one matrix per chain).  Kicks p += (eps*kick) g, drift q += (eps*drift) (imm p);
 * n_steps / step_idx as in bjx_leapfrog_diag_masked (NULL = every chain advances). */
int bjx_leapfrog_dense_coef(void* stream, int64_t N, int64_t D, int n_kicks, float kick_a, float kick_b,
                            float drift, float eps, const float* eps_per_chain, const float* imm,
                            int64_t matrix_stride, const float* q_in, const float* p_in, const float* g,
                            float* q_out, float* p_out, const int32_t* n_steps, int32_t step_idx);

int bjx_hmc_finish_dense_coef(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                              int64_t step_fold, int64_t N, int64_t D, float kick_coef, float eps,
                              const float* eps_per_chain, const float* imm, int64_t matrix_stride,
                              float divergence_threshold, const float* q0, const float* logp0,
                              const float* g0, const float* ke0, const float* q1, const float* logp1,
                              const float* g1, const float* p, float* p1_work, float* v_work,
                              float* p_end_out, float* q_out, float* logp_out, float* g_out,
                              float* acceptance_rate_out, uint8_t* is_accepted_out,
                              uint8_t* is_divergent_out, float* energy_out);

/* A WHOLE HMC transition in one launch for a log-density the engine evaluates itself (target_kind /
 * target_vec: the BJX_TARGET_* values of bjx_nuts.h) -- momentum draw, num_integration_steps velocity-Verlet
 * leapfrogs with (logp, grad) computed in registers, energies, Metropolis accept, select.  NOT the reference's
 * contract (blackjax.hmc calls logdensity_fn between two leapfrogs, hmc.py:279-312): an opt-in path that shows
 * what the contract costs; bit for bit the results of bjx_hmc_momentum_kick_diag + the target kernel +
 * bjx_leapfrog_diag + bjx_hmc_finish_diag.  Diagonal metric, 128 < D <= 1024, D % 4 == 0.
 * p0_out (HMCInfo.momentum) and q1_out / p_end_out / logp1_out / g1_out (HMCInfo.proposal) may each be NULL. */
int bjx_hmc_trajectory_diag(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                            int64_t step_fold, int64_t N, int64_t D, int64_t num_integration_steps,
                            float eps, const float* eps_per_chain, const float* imm, int64_t imm_stride,
                            float divergence_threshold, int32_t target_kind, const float* target_vec,
                            const float* q0, const float* logp0, const float* g0, float* p0_out,
                            float* q1_out, float* p_end_out, float* logp1_out, float* g1_out, float* q_out,
                            float* logp_out, float* g_out, float* acceptance_rate_out,
                            uint8_t* is_accepted_out, uint8_t* is_divergent_out, float* energy_out);

/* One step of multinomial HMC after the callable, dense metric: closing half kick p1 = p + (eps/2) g
 * [-> p1_work], v1 = imm p1 [-> v_work], then energy, weight, divergence flag, progressive uniform
 * sampling with key fold_in(integrator_key, step) and the reservoir copy of (q, p1, g).  The caller
 * continues the trajectory from p1_work with bjx_leapfrog_dense(_coef) and n_kicks = 1. */
int bjx_mhmc_step_dense(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                        int64_t step_fold, int64_t N, int64_t D, int64_t step, float eps,
                        const float* eps_per_chain, const float* imm, int64_t matrix_stride,
                        float divergence_threshold, const float* logp0, const float* ke0, const float* q,
                        const float* p, const float* g, const float* logp_new, float* p1_work,
                        float* v_work, float* weight, float* sum_log_p_accept, uint8_t* any_divergent,
                        uint8_t* ever_accepted, float* prop_q, float* prop_p, float* prop_g,
                        float* prop_logp, float* prop_energy);

/* bjx_mhmc_step_dense with per-chain trajectory lengths (blackjax.dmhmc with a dense metric: blackjax/__init__.py
 * 155-163 over mcmc/dynamic_hmc.py:85-118): chain r takes part in step `step` only while step < n_steps[r];
 * otherwise its momentum is copied to p1_work unchanged and its reservoir is left alone.  Continue with
 * bjx_leapfrog_dense_coef(..., n_steps, step + 1). */
int bjx_mhmc_step_dense_masked(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                               int64_t step_fold, int64_t N, int64_t D, int64_t step, float eps,
                               const float* eps_per_chain, const float* imm, int64_t matrix_stride,
                               float divergence_threshold, const float* logp0, const float* ke0, const float* q,
                               const float* p, const float* g, const float* logp_new, float* p1_work,
                               float* v_work, float* weight, float* sum_log_p_accept, uint8_t* any_divergent,
                               uint8_t* ever_accepted, float* prop_q, float* prop_p, float* prop_g,
                               float* prop_logp, float* prop_energy, const int32_t* n_steps);

/* bjx_mhmc_step_dense[_masked] for any palindromic integrator [b1, a1, ..., b1] (integrators.py:104-150, 335-369):
 * the closing kick of a leapfrog is p1 = p + (eps kick_coef) g with kick_coef = b1 (1/2 = velocity Verlet);
 * n_steps may be NULL (all chains take part: blackjax.mhmc) or per-chain trajectory lengths (blackjax.dmhmc).
 * The opening stage and the stages in between are bjx_leapfrog_dense_coef launches (round 4). */
int bjx_mhmc_step_dense_coef(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                             int64_t step_fold, int64_t N, int64_t D, int64_t step, float kick_coef, float eps,
                             const float* eps_per_chain, const float* imm, int64_t matrix_stride,
                             float divergence_threshold, const float* logp0, const float* ke0, const float* q,
                             const float* p, const float* g, const float* logp_new, float* p1_work,
                             float* v_work, float* weight, float* sum_log_p_accept, uint8_t* any_divergent,
                             uint8_t* ever_accepted, float* prop_q, float* prop_p, float* prop_g,
                             float* prop_logp, float* prop_energy, const int32_t* n_steps);

/* Closing half kick + energies + Metropolis accept + select with a dense metric (same contract as
 * bjx_hmc_finish_diag).  p1_work, v_work: (N, D) scratch (p1_work must not alias p). */
int bjx_hmc_finish_dense(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                         int64_t step_fold, int64_t N, int64_t D, float eps,
                         const float* eps_per_chain, const float* imm, float divergence_threshold,
                         const float* q0, const float* logp0, const float* g0, const float* ke0,
                         const float* q1, const float* logp1, const float* g1, const float* p,
                         float* p1_work, float* v_work, float* p_end_out, float* q_out,
                         float* logp_out, float* g_out, float* acceptance_rate_out,
                         uint8_t* is_accepted_out, uint8_t* is_divergent_out, float* energy_out);

/* ---- PER-CHAIN dense metric: one (D, D) inverse mass matrix per chain, (N, D, D) row-major ----
 * This is what a vmapped `window_adaptation(..., is_mass_matrix_diagonal=False).run` produces in
 * the reference.  Batched matrix-vector products with fp64 accumulation (bound by reading D^2
 * words per chain, not by MFMA).  Same contracts as the shared-matrix entry points above.
 *
 * y[c][i] = sum_j M[c][j][i] * x[c][j]   (M^T x per chain; the building block). */
int bjx_pc_matvec_t(void* stream, int64_t N, int64_t D, const float* M, int64_t matrix_stride,
                    const float* x, float* y);
/* matrix_stride = D*D for (N, D, D) per-chain matrices, 0 to apply ONE (D, D) matrix to every chain
 * through the same fp64-accumulated kernels (used by NUTS with a shared dense metric, where
 * bit-compatibility with the oracle matters more than MFMA throughput). */
int bjx_hmc_momentum_dense_pc(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                              int64_t step_fold, int64_t N, int64_t D, const float* mass_sqrt_t,
                              const float* imm, int64_t matrix_stride, float* z_work, float* v_work,
                              float* p_out, float* ke_out);
/* p_out may alias p_in here (each element is read and written by the same lane). */
int bjx_leapfrog_dense_pc(void* stream, int64_t N, int64_t D, int n_kicks, float eps,
                          const float* eps_per_chain, const float* imm, int64_t matrix_stride,
                          const float* q_in, const float* p_in, const float* g, float* q_out,
                          float* p_out);
int bjx_hmc_finish_dense_pc(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset,
                            int64_t step_fold, int64_t N, int64_t D, float eps,
                            const float* eps_per_chain, const float* imm, int64_t matrix_stride,
                            float divergence_threshold, const float* q0, const float* logp0,
                            const float* g0, const float* ke0, const float* q1, const float* logp1,
                            const float* g1, const float* p, float* p1_work, float* v_work,
                            float* p_end_out, float* q_out, float* logp_out, float* g_out,
                            float* acceptance_rate_out, uint8_t* is_accepted_out,
                            uint8_t* is_divergent_out, float* energy_out);

/* Welford with a dense second-moment matrix per chain: m2 (N, D, D) += outer(value - mean_new,
 * value - mean_old).  Replaces: blackjax/adaptation/mass_matrix.py:424-435 (dense branch). */
int bjx_welford_update_dense(void* stream, int64_t N, int64_t D, int64_t sample_size_new,
                             const float* value, const float* mean_in, const float* m2_in,
                             float* mean_out, float* m2_out);
/* Window end (dense): imm = (n/(n+5+k)) m2/(n-1) + (k/(n+5+k)) imm_prev + (5/(n+5+k)) 1e-3 I.
 * imm_prev is (D, D) [imm_prev_per_chain = 0] or (N, D, D) [= 1].  Replaces: mass_matrix.py:335-357. */
int bjx_welford_final_dense(void* stream, int64_t N, int64_t D, int64_t sample_size,
                            float imm_shrinkage_to_previous, const float* m2, const float* imm_prev,
                            int imm_prev_per_chain, float* imm_out);

/* ---- window adaptation (per-chain state; every array is (N,) unless noted) ------------------
 *
 * Dual averaging init (from_log_avg = 0: x = x_in) or window-end re-init (from_log_avg = 1:
 * x = exp(x_in) with x_in = log_step_size_avg):
 *   mu = log(10 x) ; log_x = log(x) ; log_x_avg = 0 ; avg_error = 0 ; step_size = exp(log_x)
 * Replaces: blackjax/optimizers/dual_averaging.py:87-99 ; adaptation/staged_adaptation.py:242-243. */
int bjx_da_init(void* stream, int64_t N, int from_log_avg, const float* x_in, float* log_x_out,
                float* log_x_avg_out, float* avg_error_out, float* mu_out, float* step_size_out);

/* One dual-averaging update with gradient = target - acceptance_rate (`step` >= 1 is the
 * reference's DualAveragingState.step, identical for all chains); outputs may alias inputs.
 *   reg = step + t0 ; eta = step^-kappa ; avg_error = (1 - 1/reg) avg_error + g/reg
 *   log_x = mu - (sqrt(step)/gamma) avg_error ; log_x_avg = eta log_x_prev + (1-eta) log_x_avg
 *   step_size = exp(log_x)
 * Replaces: dual_averaging.py:101-123 ; adaptation/step_size.py:129-145 ;
 * staged_adaptation.py:186-198. */
int bjx_da_update(void* stream, int64_t N, int64_t step, float target, float t0, float gamma,
                  float kappa, const float* acceptance_rate, const float* log_x_in,
                  const float* log_x_avg_in, const float* avg_error_in, const float* mu,
                  float* log_x_out, float* log_x_avg_out, float* avg_error_out,
                  float* step_size_out);

/* y = exp(x) element-wise, fp64 rounded once (final step size exp(log_step_size_avg),
 * staged_adaptation.py:301-305). */
int bjx_exp(void* stream, int64_t N, const float* x, float* y);

/* Welford accumulation of one new sample per chain, diagonal: value/mean/m2 are (N, D);
 * sample_size_new is the count AFTER adding this sample.  Outputs may alias inputs.
 * Replaces: blackjax/adaptation/mass_matrix.py:288-291,410-435. */
int bjx_welford_update_diag(void* stream, int64_t N, int64_t D, int64_t sample_size_new,
                            const float* value, const float* mean_in, const float* m2_in,
                            float* mean_out, float* m2_out);

/* Window end: imm = (n/(n+5+k)) m2/(n-1) + (k/(n+5+k)) imm_prev + (5/(n+5+k)) 1e-3, k =
 * imm_shrinkage_to_previous.  imm_prev is (D,) [stride 0] or (N, D) [stride D]; imm_out (N, D).
 * Replaces: mass_matrix.py:335-357,437-442. */
int bjx_welford_final_diag(void* stream, int64_t N, int64_t D, int64_t sample_size,
                           float imm_shrinkage_to_previous, const float* m2, const float* imm_prev,
                           int64_t imm_prev_stride, float* imm_out);

/* ---- MALA (blackjax.mala; blackjax/mcmc/mala.py) --------------------------------------------
 * One transition = bjx_mala_propose -> user callable at q1 -> bjx_mala_finish.  `tau` is the step size
 * (scalar, or a device (N,) array `tau_per_chain` as with `eps`).  Keys as in bjx_hmc_finish_diag:
 *   k_i = split(key, .)[chain_offset+i] (or its step_fold child) ; key_integrator, key_rmh = split(k_i, 2)
 *
 * Proposal: q1 = q0 + tau g0 + sqrt(2 tau) normal(key_integrator, (D,)), left to right, one fma per term.
 * Replaces: mcmc/diffusions.py::overdamped_langevin (one_step) as called by mcmc/mala.py (kernel). */
int bjx_mala_propose(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                     int64_t N, int64_t D, float tau, const float* tau_per_chain, const float* q0,
                     const float* g0, float* q1_out);
/* Asymmetric Metropolis-Hastings accept + state select, out of place:
 *   E(a -> b) = -logp_b + (0.25 * (1 / tau)) * sum (q_a - q_b - tau g_b)^2      (transition_energy)
 *   delta = E(q1 -> q0) - E(q0 -> q1) (NaN -> -inf) ; p_acc = min(1, exp(delta))
 *   accept = uniform(key_rmh) < p_acc ; (q, logp, g)_out = accept ? (q1, logp1, g1) : (q0, logp0, g0)
 * is_accepted_out: one byte per chain, 0 / 1.
 * Replaces: mcmc/mala.py (transition_energy, kernel) ; mcmc/proposal.py::compute_asymmetric_acceptance_ratio,
 * static_binomial_sampling, safe_energy_diff. */
int bjx_mala_finish(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                    int64_t N, int64_t D, float tau, const float* tau_per_chain, const float* q0,
                    const float* logp0, const float* g0, const float* q1, const float* logp1, const float* g1,
                    float* q_out, float* logp_out, float* g_out, float* acceptance_rate_out,
                    uint8_t* is_accepted_out);

/* ---- Periodic orbital (blackjax.orbital_hmc; blackjax/mcmc/periodic_orbital.py) -------------
 * The state of a chain is a weighted orbit of P slots: positions / grads (N, P, D) = (N * P, D) rows, weights /
 * logdensities (N, P), directions (N, P) int32.  One transition = bjx_orbital_open -> user callable on the (N * P, D)
 * rows of q_out -> bjx_orbital_finish.  `eps` is the step size (scalar, or a device (N,) array `eps_per_chain`), `imm`
 * the diagonal inverse mass matrix ((D,) with imm_stride 0, or (N, D) with imm_stride D), as in bjx_leapfrog_diag.  Keys:
 *   k_i = split(key, .)[chain_offset+i] (or its step_fold child) ; key_momentum, key_select = split(k_i, 2)
 * Outputs are out of place: no output may alias an input.  N == 0 is a no-op.
 *
 * Opening, per chain:
 *   cum_j = cumsum(weights)_j (each prefix in fp64, rounded once) ; r = cum_{P-1} * (1 - uniform(key_select)) in fp32
 *   i = #{j : cum_j < r}, at most P - 1 ; choice_out = i ; (q, logp, g) = slot i ; d = directions[i]
 *   p = (1 / sqrt(imm)) * normal(key_momentum, (D,))                          (drawn once, as bjx_hmc_momentum_diag)
 * and for every slot j = 0 .. P-1:  step_out[j] = s_j = float(j - d) * eps  (an fp32 product) and
 *   drift = 1:  p_out[j] = p_half = fma(s_j / 2, g, p) ;  q_out[j] = fma(s_j, imm * p_half, q)
 *   drift = 0:  p_out[j] = p ;  q_out[j] = q                     (the selected state repeated: a user bijection's input)
 * logp_rep_out (N * P,) / g_rep_out (N * P, D), where not NULL, receive the selected logp / g repeated.
 * q_out, p_out: (N * P, D); step_out: (N * P,); choice_out: (N,) int32.
 * Replaces: jax/_src/random.py::choice ; mcmc/metrics.py::gaussian_euclidean (sample_momentum) ;
 * mcmc/periodic_orbital.py::periodic_orbital_proposal (generate) with mcmc/integrators.py::velocity_verlet up to its
 * log-density evaluation. */
int bjx_orbital_open(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                     int64_t P, int64_t D, int drift, float eps, const float* eps_per_chain, const float* imm,
                     int64_t imm_stride, const float* weights, const int32_t* directions, const float* positions,
                     const float* logdensities, const float* grads, float* q_out, float* p_out, float* step_out,
                     int32_t* choice_out, float* logp_rep_out, float* g_rep_out);
/* Closing, per chain and slot j, with (logp_j, g_j) the callable's outputs at q_out[j] and s_j = step[j]:
 *   kick = 1:  momentums_out[j] = p_j = fma(s_j / 2, g_j, p_in[j])   (the closing half kick of velocity_verlet)
 *   kick = 0:  momentums_out[j] = p_j = p_in[j]                      (a user bijection's momentum; g may be NULL)
 *   logw_j = logp_j - 0.5 * dot(imm * p_j, p_j)   (fp64 dot rounded once, fp32 subtraction; NaN or +inf -> -inf)
 * then over the P slots:  m = max logw ; e_j = exp(logw_j - m) (fp64, rounded once) ; S = sum e (fp64, rounded once)
 *   weights_out[j] = e_j / S ; weights_mean_out = mean(w) ; weights_variance_out = mean((w - mean(w))^2), both fp64
 *   sums rounded once ; directions_out[j] = j
 * Replaces: mcmc/periodic_orbital.py::periodic_orbital_proposal (generate: the weights) and kernel (the info), with
 * mcmc/metrics.py::gaussian_euclidean (kinetic_energy) and jax.nn.softmax. */
int bjx_orbital_finish(void* stream, int64_t N, int64_t P, int64_t D, int kick, const float* imm,
                       int64_t imm_stride, const float* step, const float* p_in, const float* logp, const float* g,
                       float* momentums_out, float* weights_out, int32_t* directions_out, float* weights_mean_out,
                       float* weights_variance_out);

/* ---- marginal latent Gaussian (blackjax.mgrad_gaussian; blackjax/mcmc/marginal_latent_gaussian.py) ----
 * Gaussian prior N(0, C), C = U diag(Gamma) U^T shared by all chains, arbitrary log-LIKELIHOOD with a gradient (a
 * prior mean is folded into the likelihood: bjx_mgrad_shift).  The kernels work on rows in the prior's eigenbasis,
 * U_x = U^T x and U_grad_x = U^T g; the rotations are the caller's GEMMs.  One transition of a dense prior =
 *   bjx_mgrad_propose -> bjx_dense_matmul(t, U^T) = y -> user callable at y [-> bjx_mgrad_shift]
 *   -> bjx_dense_matmul_bt(y, U, U^T) = U_y -> bjx_dense_matmul_bt(g_y, U, U^T) = U_grad_y -> bjx_mgrad_finish
 * and of a diagonal prior (U = I, Gamma = the variances) propose -> user callable at t [-> shift] -> finish.
 * `delta` is the step size (scalar, or a device (N,) array `delta_per_chain` as with `eps`); `gamma` is (D,).  Keys:
 *   k_i = split(key, .)[chain_offset+i] (or its step_fold child) ; y_key, u_key = split(k_i, 2)
 * Per element, in fp32 left to right with correctly rounded divisions:
 *   Gamma_1 = Gamma delta / (delta + 2 Gamma) ; Gamma_3 = (delta + 2 Gamma) / (delta + 4 Gamma) ; Gamma_2 = Gamma_1 / Gamma_3
 * Outputs are out of place: no output may alias an input.  N == 0 is a no-op.
 *
 * Proposal: t = Gamma_1 (U_x / (0.5 delta) + U_grad_x) + sqrtf(Gamma_2) normal(y_key, (D,)), the sum one fma.
 * Replaces: mcmc/marginal_latent_gaussian.py (build_kernel: kernel, up to y = U @ ...). */
int bjx_mgrad_propose(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                      int64_t N, int64_t D, float delta, const float* delta_per_chain, const float* gamma,
                      const float* u_x, const float* u_grad_x, float* t_out);
/* logp_out = logp + dot(y, shift) (fp64 sum rounded once) ; g_out = g + shift, with shift = C^-1 mean (D,).
 * Replaces: mcmc/marginal_latent_gaussian.py::generate_mean_shifted_logprob and its gradient. */
int bjx_mgrad_shift(void* stream, int64_t N, int64_t D, const float* shift, const float* y, const float* logp,
                    const float* g, float* logp_out, float* g_out);
/* Metropolis-Hastings accept + state select, out of place:
 *   t_x = Gamma_1 (U_x / (0.5 delta) + 0.5 U_grad_x) ; t_y = Gamma_1 (U_y / (0.5 delta) + 0.5 U_grad_y)
 *   hxy = sum (U_x - t_y) (Gamma_3 U_grad_y) ; hyx = sum (U_y - t_x) (Gamma_3 U_grad_x)   (fp64 sums, rounded once)
 *   log_ratio = ((logp_y - logp_x) + hxy) - hyx (NaN -> -inf) ; p_acc = min(1, exp(log_ratio))
 *   accept = uniform(u_key) < p_acc ; (x, logp, g, U_x, U_grad_x)_out = accept ? the proposal's : the state's
 * Dense prior: x, g_x, y, g_y, x_out, g_out are all given.  Diagonal prior: all six are NULL -- position and gradient
 * ARE u_x / u_grad_x (u_y / u_grad_y for the proposal) and are written once, to u_x_out / u_grad_x_out.
 * is_accepted_out: one byte per chain, 0 / 1.
 * Replaces: mcmc/marginal_latent_gaussian.py (build_kernel: kernel, from hxy on) ; mcmc/proposal.py::
 * static_binomial_sampling, safe_energy_diff. */
int bjx_mgrad_finish(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                     int64_t D, float delta, const float* delta_per_chain, const float* gamma, const float* x,
                     const float* logp_x, const float* g_x, const float* u_x, const float* u_grad_x, const float* y,
                     const float* logp_y, const float* g_y, const float* u_y, const float* u_grad_y, float* x_out,
                     float* logp_out, float* g_out, float* u_x_out, float* u_grad_x_out, float* acceptance_rate_out,
                     uint8_t* is_accepted_out);

/* ---- SGMCMC (blackjax.sgld / sghmc / sgnht / csgld; blackjax/sgmcmc/) -------------------------
 * Stochastic-gradient samplers: the gradient estimate `g` comes from the caller (a minibatch gradient), a step is
 * one launch that draws its normals in registers.  `eps` is the step size and `temperature` the temperature, each a
 * scalar or a device (N,) array (`*_per_chain`, which wins when non-null).  Outputs are out of place: no output may
 * alias an input.  Keys: k_i = split(key, .)[chain_offset+i] (or its step_fold child), used unsplit for the noise
 * of SGLD and SGNHT.  Nothing tests for non-finite values.  N == 0 is a no-op.
 *
 * SGLD: q1 = q + eps g + sqrtf((2 T) eps) normal(k_i, (D,)), left to right, one fma per term.
 * Replaces: sgmcmc/diffusions.py::overdamped_langevin (one_step) as called by sgmcmc/sgld.py (kernel). */
int bjx_sgld_step(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                  int64_t D, float eps, const float* eps_per_chain, float temperature,
                  const float* temperature_per_chain, const float* q, const float* g, float* q_out);
/* SGHMC, integration step `step_index` = l of L (one launch per step; the caller evaluates g_l at q_l between):
 *   q_{l+1} = q_l + eps p_l
 *   p_{l+1} = (1 - alpha eps) p_l + eps g_l + s normal(split(k_i, L)[l], (D,)),  s = sqrtf((eps T)(2 alpha - eps beta))
 * with c = 1 - alpha eps two fp32 roundings, c p_l one rounding, then one fma per term.
 *   p_in == NULL: p_l is the momentum refresh normal(k_i, (D,)), drawn in registers (l = 0).
 *   g == NULL and p_out == NULL: only q_{l+1} is written and no noise is drawn (l = L - 1; the sampler drops the
 *   final momentum).  g and p_out must be null together.  Both forms at once serve L = 1.
 * Replaces: sgmcmc/sghmc.py (kernel: momentum refresh, integration loop) ; sgmcmc/diffusions.py::sghmc (one_step). */
int bjx_sghmc_step(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, int64_t step_index, float alpha, float beta, float eps, const float* eps_per_chain,
                   float temperature, const float* temperature_per_chain, const float* q, const float* p_in,
                   const float* g, float* q_out, float* p_out);
/* SGNHT, with z = normal(k_i, (D,)) and s as for SGHMC; xi is the (N,) thermostat:
 *   q1 = q + eps p ; p1 = ((p - (eps xi) p) + eps g) + s z, one fma per term
 *   xi1 = xi + eps (m - T), m = sum_j p1_j^2 / D accumulated in fp64 and rounded once
 * Replaces: sgmcmc/diffusions.py::sgnht (one_step) as called by sgmcmc/sgnht.py (kernel). */
int bjx_sgnht_step(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, float alpha, float beta, float eps, const float* eps_per_chain, float temperature,
                   const float* temperature_per_chain, const float* q, const float* p, const float* xi,
                   const float* g, float* q_out, float* p_out, float* xi_out);
/* Contour SGLD, the position half.  energy_pdf is the (N, M) per-chain energy histogram and energy_idx the (N,)
 * int32 index of each chain's current energy bin, clamped into [1, M - 1] on read.  Per chain, in fp32 in this order
 * (each log in fp64 rounded once):
 *   m = 1 + (((zeta T) (log pdf[i] - log pdf[i - 1])) / energy_gap)
 *   q1 = q + eps (m g) + sqrtf((2 T) eps) normal(k_i, (D,)),  m g one rounding, then one fma per term
 * A non-positive histogram entry gives a NaN row.  "bad sizes" also covers M < 2.
 * Replaces: the multiplier of sgmcmc/csgld.py (kernel) and its call of sgmcmc/diffusions.py::overdamped_langevin. */
int bjx_csgld_step(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, int64_t M, float zeta, float energy_gap, float eps, const float* eps_per_chain,
                   float temperature, const float* temperature_per_chain, const float* q, const float* g,
                   const float* energy_pdf, const int32_t* energy_idx, float* q_out);
/* Contour SGLD, the histogram half, from logdensity (N,), the log-density estimate at the new position:
 *   x = floorf(((-logdensity - min_energy) / energy_gap) + 1) ; i = !(x >= 1) ? 1 : (x >= M - 1 ? M - 1 : (int)x)
 *   w = eps_sa * pdf_in[i]^zeta   (pow in fp64 rounded once; zeta == 1: pdf_in[i] itself)
 *   pdf_out[j] = fma(w, (j == i ? 1 - pdf_in[j] : -pdf_in[j]), pdf_in[j]) ; idx_out = i
 * NaN and -inf energies give i = 1, +inf gives M - 1.  eps_sa is a scalar or (N,) as eps above.
 * Replaces: the index and stochastic-approximation update of sgmcmc/csgld.py (kernel). */
int bjx_csgld_update(void* stream, int64_t N, int64_t M, float zeta, float energy_gap, float min_energy, float eps_sa,
                     const float* eps_sa_per_chain, const float* logdensity, const float* pdf_in, float* pdf_out,
                     int32_t* idx_out);

/* ---- Barker (blackjax.barker_proposal; blackjax/mcmc/barker.py) ------------------------------
 * One transition = bjx_barker_propose -> user callable at q1 -> bjx_barker_finish.  `tau` as for MALA.  `imm` is a
 * diagonal inverse mass matrix: null = ones, (D,) with imm_row_stride 0, or (N, D) with imm_row_stride D.  Keys:
 *   k_i = split(key, .)[chain_offset+i] (or its step_fold child) ; key_sample, key_rmh = split(k_i, 2) ;
 *   k1, k2 = split(key_sample, 2)
 *
 * Proposal, per element d (each product one fp32 rounding, expit in fp64 rounded once):
 *   z = (tau * sqrtf(imm[d])) * normal(k1, (D,))[d] ; p = expit(z * g0[d]) ; b = uniform(k2, (D,))[d] < p
 *   q1[d] = b ? q0[d] + z : q0[d] - z          (a NaN p compares false)
 * Replaces: mcmc/barker.py::_barker_sample_nd as called by its kernel, diagonal preconditioner. */
int bjx_barker_propose(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                       int64_t N, int64_t D, float tau, const float* tau_per_chain, const float* imm,
                       int64_t imm_row_stride, const float* q0, const float* g0, float* q1_out);
/* Asymmetric Metropolis-Hastings accept + state select, out of place.  With t = q1 - q0 (the diagonal scale
 * cancels, so neither tau nor imm is needed) and softplus(x) = max(x, 0) + log1p(exp(-|x|)) in fp64:
 *   S = sum_d softplus(-(t g0)) - softplus(t g1)   (fp64 sum, rounded once)
 *   log_ratio = (logp1 - logp0) + S (NaN -> -inf) ; p_acc = min(1, exp(log_ratio))
 *   accept = uniform(key_rmh) < p_acc ; (q, logp, g)_out = accept ? (q1, logp1, g1) : (q0, logp0, g0)
 * is_accepted_out: one byte per chain, 0 / 1.
 * Replaces: mcmc/barker.py (_barker_logpdf, kernel) ; mcmc/proposal.py::compute_asymmetric_acceptance_ratio,
 * static_binomial_sampling, safe_energy_diff. */
int bjx_barker_finish(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold,
                      int64_t N, int64_t D, const float* q0, const float* logp0, const float* g0,
                      const float* q1, const float* logp1, const float* g1, float* q_out, float* logp_out,
                      float* g_out, float* acceptance_rate_out, uint8_t* is_accepted_out);

/* ---- elliptical slice (blackjax.elliptical_slice; blackjax/mcmc/elliptical_slice.py) ----------
 * Gaussian prior N(mean, cov) shared by all chains, arbitrary log-LIKELIHOOD (value only, no gradient).  One
 * transition = bjx_ess_begin -> user callable at q_prop -> { bjx_ess_shrink -> user callable at q_prop } until
 * bjx_ess_shrink leaves *n_live == 0.  Keys:
 *   k_i = split(key, .)[chain_offset+i] (or its step_fold child) ;
 *   key_slice, key_momentum, key_uniform, key_theta = split(k_i, 4)
 * With c, s = cos, sin of (double)theta, each rounded once, a = q0 - mean and b = nu - mean:
 *   p(theta) = fma(b, s, a * c) + mean ;  m(theta) = fma(-a, s, b * c) + mean            (ellipsis)
 *
 * bjx_ess_begin: exactly one of cov_diag (D,) and nu_lin (N, D) is given.
 *   nu = fma(sqrtf(cov_diag[j]), normal(key_momentum, (D,))[j], mean[j])                 (diagonal prior)
 *   nu = nu_lin + mean, nu_lin = normal(key_momentum, (D,)) @ L^T from bjx_ess_noise + bjx_dense_matmul   (dense)
 *   logy = logp0 + log(uniform(key_uniform))   (fp64 log rounded once; u = 0 gives -inf)
 *   theta = f32(2 pi) * uniform(key_theta) ; theta_min = theta - f32(2 pi) ; theta_max = theta
 *   q_prop = p(theta) ; subiter = 1 ; done = 0
 * Replaces: mcmc/elliptical_slice.py (kernel, elliptical_proposal up to its while_loop), util.py::generate_gaussian_noise. */
int bjx_ess_begin(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                  int64_t D, const float* mean, const float* cov_diag, const float* nu_lin, const float* q0,
                  const float* logp0, float* nu_out, float* q_prop_out, float* logy_out, float* theta_out,
                  float* theta_min_out, float* theta_max_out, int32_t* subiter_out, uint8_t* done_out);
/* n_out[i] = normal(key_momentum of chain i, (D,)): the left operand of the dense prior's product. */
int bjx_ess_noise(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                  int64_t D, float* n_out);
/* One round of the reference's while_loop (slice_fn), given logp_prop = log-likelihood of every q_prop row.  Per row:
 *   done set: skipped (one byte read).
 *   !(logp_prop <= logy) (a NaN ends the loop, as in the reference): logdensity_out = logp_prop, theta_out = theta,
 *     subiter_out = subiter, momentum_out = m(theta), done = 1.  The q_prop row is the chain's new position and is
 *     not written again.
 *   otherwise: theta = max(theta_min, fma(unit_float(bits), theta_max - theta_min, theta_min)), bits from
 *     fold_in(key_slice, subiter) ; q_prop = p(theta) ; theta_min = theta if theta < 0 ; theta_max = theta if
 *     theta > 0 ; subiter += 1 ; *n_live += 1 (one atomic per row).
 * The caller zeroes *n_live on the stream before the launch; there is no cap on the number of rounds here. */
int bjx_ess_shrink(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, const float* mean, const float* q0, const float* nu, const float* logp_prop,
                   const float* logy, float* theta, float* theta_min, float* theta_max, int32_t* subiter,
                   uint8_t* done, float* q_prop, float* logdensity_out, float* theta_out, int32_t* subiter_out,
                   float* momentum_out, int32_t* n_live);

/* ---- random walk (blackjax.rmh / additive_step_random_walk / irmh; blackjax/mcmc/random_walk.py, irmh.py) ----
 * Gradient-free Metropolis-Hastings.  One transition = a proposal (bjx_rw_propose, or a user generator) -> user
 * callable at q1, VALUE ONLY -> bjx_rw_finish.  Keys:
 *   k_i = split(key, .)[chain_offset+i] (or its step_fold child) ; key_proposal, key_accept = split(k_i, 2)
 *
 * out[i] = normal(k, (D,)) with k = k_i (child == -1) or split(k_i, 2)[child] (child 0 or 1): what
 * random.chain_normal hands a user-written generator, and the left operand of the dense step's product. */
int bjx_rw_noise(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int32_t child,
                 int64_t N, int64_t D, float* out);
/* The Gaussian random step added to the position, out of place.  At most one of sigma_diag (D,) and move_lin (N, D):
 *   q1 = fma(s_j, normal(key_proposal, (D,))[j], q0), s_j = sigma_diag[j] or the scalar sigma    (scalar / diagonal)
 *   q1 = q0 + move_lin, move_lin = normal(key_proposal, (D,)) @ sigma^T from bjx_rw_noise(child 0) +
 *        bjx_dense_matmul, i.e. row i = sigma @ z_i                                               (dense)
 * Replaces: mcmc/random_walk.py::normal (propose) and build_additive_step (the sum), util.py::generate_gaussian_noise. */
int bjx_rw_propose(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                   int64_t D, float sigma, const float* sigma_diag, const float* move_lin, const float* q0,
                   float* q1_out);
/* Metropolis-Hastings accept + state select, out of place.  f_init_prop[i] = log-density of proposing q1 from q0,
 * f_prop_init[i] = of proposing q0 from q1; both null for a symmetric proposal (exactly one null is an error):
 *   e_init = (-logp0) - f_init_prop ; e_new = (-logp1) - f_prop_init         (transition_energy; -logp without f)
 *   delta = e_init - e_new (NaN -> -inf) ; p_acc = min(1, exp(delta))
 *   accept = uniform(key_accept) < p_acc ; (q, logp)_out = accept ? (q1, logp1) : (q0, logp0)
 * Only the chosen source row is read.  is_accepted_out: one byte per chain, 0 / 1.
 * Replaces: mcmc/random_walk.py::build_rmh (transition_energy, kernel, rmh_proposal), mcmc/irmh.py::build_kernel ;
 * mcmc/proposal.py::compute_asymmetric_acceptance_ratio, static_binomial_sampling, safe_energy_diff. */
int bjx_rw_finish(void* stream, uint32_t key0, uint32_t key1, int64_t chain_offset, int64_t step_fold, int64_t N,
                  int64_t D, const float* q0, const float* logp0, const float* q1, const float* logp1,
                  const float* f_init_prop, const float* f_prop_init, float* q_out, float* logp_out,
                  float* acceptance_rate_out, uint8_t* is_accepted_out);

/* ---- SMC (blackjax.tempered_smc / adaptive_tempered_smc; blackjax/smc/) -----------------------
 * One step = bjx_smc_resample -> bjx_smc_gather -> num_mcmc_steps transitions of an MCMC kernel on the tempered
 * log-density (bjx_smc_temper after the two user callables) -> user log-likelihood -> bjx_smc_reweight; the adaptive
 * sampler first runs bjx_smc_ess_solve.  Temperatures travel as device scalars: no entry point reads anything back.
 *
 * Resampling.  Cumulative weights in 2^-62 fixed point: wf_j = (int64) floor((double) w_j * 2^62) (w_j clamped to
 * [0, 1], NaN = 0), C = inclusive prefix sum (integer, so independent of the tiling: tiles of bjx_smc_scan_tile()
 * items, launch-separated -- tile sums, scan of the tile sums, apply; no workgroup waits on another).
 *   pos_i = ((float) i + u_i) / (float) num_samples                       (fp32)
 *   u_i = uniform(key, ()) [systematic] or uniform(key, (num_samples,))[i] [stratified != 0]
 *   ancestors_out[i] = min(N - 1, #{j : C_j < (int64)((double) pos_i * 2^62)})
 * 1 <= N <= 2^24, num_samples <= 2^24 (positions are fp32).  workspace: bjx_smc_resample_workspace_bytes(N) bytes
 * (0 for an N out of range), 8-byte aligned.
 * Replaces: smc/resampling.py::systematic, stratified (searchsorted on cumsum + clip). */
int bjx_smc_scan_tile(void);
int64_t bjx_smc_resample_workspace_bytes(int64_t N);
int bjx_smc_resample(void* stream, uint32_t key0, uint32_t key1, int32_t stratified, int64_t N,
                     int64_t num_samples, const float* weights, int64_t* workspace, int32_t* ancestors_out);
/* out[i, :] = x[ancestors[i], :], x (N, D), out (num_samples, D), out of place; 16-byte accesses when D % 4 == 0 and
 * both arrays are 16-byte aligned.  An index outside [0, N) is clamped into it.
 * Replaces: smc/base.py::step (the tree_map of particles[resampling_idx]). */
int bjx_smc_gather(void* stream, int64_t N, int64_t num_samples, int64_t D, const float* x,
                   const int32_t* ancestors, float* out);
/* Tempered log-posterior and gradient from the two callables' outputs, lam read from device memory:
 *   logp_out = logprior + lam * loglik ; grad_out = logprior_grad + lam * loglik_grad
 * product rounded, then sum rounded (no fused multiply-add).
 * Replaces: smc/tempered.py::build_kernel (tempered_logposterior_fn) under jax.value_and_grad. */
int bjx_smc_temper(void* stream, int64_t N, int64_t D, const float* lam, const float* logprior,
                   const float* logprior_grad, const float* loglik, const float* loglik_grad, float* logp_out,
                   float* grad_out);
/* The value alone, for samplers that take no gradient: logp_out = logprior + lam * loglik over (N,), the same
 * rounded product and rounded sum as bjx_smc_temper's logp_out (bit-equal to it).  One launch.
 * Replaces: smc/tempered.py::build_kernel (tempered_logposterior_fn). */
int bjx_smc_temper_value(void* stream, int64_t N, const float* lam, const float* logprior, const float* loglik,
                         float* logp_out);
/* lw = (*lam_new - *lam_old) * loglik (0 when the difference is 0, whatever loglik is); a NaN or -inf lw is a
 * particle of weight 0.  lse = logsumexp(lw) (fp64) ; weights_out = exp(lw - lse) ;
 * *log_likelihood_increment_out = lse - log N ; *lam_out = *lam_new.  No particle of positive weight: weights NaN,
 * increment -inf.  One workgroup.
 * Replaces: smc/tempered.py::build_kernel (log_weights_fn) ; smc/base.py::step (normalisation, increment). */
int bjx_smc_reweight(void* stream, int64_t N, const float* loglik, const float* lam_old, const float* lam_new,
                     float* weights_out, float* log_likelihood_increment_out, float* lam_out);
/* *log_ess_out = 2 logsumexp(lw) - logsumexp(2 lw), fp64 sums.  Replaces: smc/ess.py::log_ess. */
int bjx_smc_log_ess(void* stream, int64_t N, const float* log_weights, float* log_ess_out);
/* Largest temperature increment that keeps the ESS at the target, f(d) = log_ess(d * loglik) - log(N target_ess):
 *   max = *max_delta, or 1 - *lam_old when max_delta is null
 *   f(max) >= 0: delta = max ; else 30 halvings of [0, max] in fp32, left end moved to mid when f(mid) >= 0, delta =
 *   the left end (the ESS at delta is never below the target).
 * *lam_new_out (optional) = *lam_old + delta, exactly 1.0f when delta = 1 - *lam_old was taken whole.  The whole solve
 * is one launch of one workgroup.
 * Replaces: smc/ess.py::ess_solver ; smc/solver.py::dichotomy ; smc/adaptive_tempered.py::build_kernel (compute_delta). */
int bjx_smc_ess_solve(void* stream, int64_t N, const float* loglik, float target_ess, const float* max_delta,
                      const float* lam_old, float* delta_out, float* lam_new_out);

/* Multinomial and residual resampling.  Integer sums only, as above: the ancestors do not depend on the tiling.
 * Sorted uniforms (resampling.py::_sorted_uniforms, z = cumsum(-log(uniform(key, (M + 1,)))), z[:-1] / z[-1]) for
 * M = num_samples positions:
 *   u_k  = uniform(key, (M + 1,))[k]                                      (fp32, as the stratified scheme draws it)
 *   e_k  = -log1p(-u_k), correctly rounded to fp32 (bjx_log1p.h).  1 - u is as uniform as u and -u lies in (-1, 0]:
 *          e_k < 16 is finite even for a draw of exactly 0, which gives inf in the reference (a deliberate deviation)
 *   ef_k = (int64) floor((double) e_k * 2^24) ; Z = inclusive prefix sum (below 2^53: every conversion is exact)
 *   pos_i = (double) Z_i / (double) max(Z_M, 1)                           (i < M; non-decreasing)
 * mode BJX_SMC_MULTINOMIAL:  ancestors_out[i] = min(N - 1, #{j : C_j < (int64)(pos_i * 2^62)}), C as above.
 * mode BJX_SMC_RESIDUAL:  prod_j = wf_j * M exactly (86 bits) ; cnt_j = prod_j >> 62 ; rem_j = (prod_j mod 2^62) >> 24 ;
 *   Ccnt, Crem = their inclusive prefix sums ; S = Ccnt[N - 1] (never read by the host)
 *   i <  S:  ancestors_out[i] = min(N - 1, #{j : Ccnt_j <= i})                        (repeat(arange(N), cnt)[i])
 *   i >= S:  p = perm[i] (i when perm is null; clamped to [0, M)) ;
 *            ancestors_out[i] = min(N - 1, #{j : Crem_j < (int64)(pos_p * (double) Crem[N - 1])})
 *   The reference splits its key in two: (key0, key1) here is the FIRST half (the multinomial draw of the remainders);
 *   perm is jax.random.permutation(second half, M), which depends on the key alone and is formed by the caller.
 * 1 <= N <= 2^24, num_samples <= 2^24.  workspace: bjx_smc_resample_sorted_workspace_bytes(N, num_samples) bytes (0 for
 * arguments out of range), 8-byte aligned.  num_samples == 0 is a no-op.
 * Replaces: smc/resampling.py::multinomial, residual, _sorted_uniforms. */
#define BJX_SMC_MULTINOMIAL 0
#define BJX_SMC_RESIDUAL 1
int64_t bjx_smc_resample_sorted_workspace_bytes(int64_t N, int64_t num_samples);
int bjx_smc_resample_sorted(void* stream, uint32_t key0, uint32_t key1, int32_t mode, int64_t N,
                            int64_t num_samples, const float* weights, const int32_t* perm, int64_t* workspace,
                            int32_t* ancestors_out);
/* out[row0 + i * row_stride, :] = x[i, :] for i < M, x (M, D); every other row of out keeps its bytes.  The caller
 * guarantees that out has at least row0 + (M - 1) * row_stride + 1 rows.  One wavefront per row; 16-byte accesses when
 * D % 4 == 0 and both arrays are 16-byte aligned, as bjx_smc_gather.  row0 >= 0, row_stride >= 1, out of place.
 * Replaces: smc/waste_free.py::update_waste_free (the reshape of the scanned states and its concatenation). */
int bjx_smc_scatter_rows(void* stream, int64_t M, int64_t D, const float* x, int64_t row0, int64_t row_stride,
                         float* out);
/* Column means and standard deviations (ddof 0) of x (N, D), fp64 accumulators, each result rounded once.  One
 * workgroup per tile of bjx_smc_moments_tile() rows and block of columns writes the tile's (mean, sum of squared
 * deviations from it); a second launch merges the tiles in order (Chan et al.).  Launch-separated, and the tiling
 * depends on (N, D) alone: the result is reproducible bit for bit.  std_out may be null.  workspace:
 * bjx_smc_particle_moments_workspace_bytes(N, D) bytes (0 for 1 <= N <= 2^24, 1 <= D <= 2^20 violated), 8-byte aligned;
 * on return its last 2 D doubles hold the fp64 means and the fp64 sums of squared deviations.
 * Replaces: smc/tuning/from_particles.py::particles_means, particles_stds. */
int bjx_smc_moments_tile(void);
int64_t bjx_smc_particle_moments_workspace_bytes(int64_t N, int64_t D);
int bjx_smc_particle_moments(void* stream, int64_t N, int64_t D, const float* x, void* workspace, float* mean_out,
                             float* std_out);

/* Pretuning (blackjax.pretuning): a population of move parameters, one row per particle, scored by the expected
 * squared jump distance of one trial transition, jittered and resampled by that score before every SMC step.  The
 * ancestors are bjx_smc_resample_sorted's (BJX_SMC_MULTINOMIAL) from the weights below.  All three launch on the
 * caller's stream and read nothing back.  1 <= N, M <= 2^24 ; 1 <= D, K <= 2^20.
 *
 * bjx_smc_esjd:  d_j = prev[i, j] - next[i, j] (fp32) ; s_i = sum_j d_j^2 / imm_j in fp64 (imm null: all ones;
 *   otherwise imm[i * imm_stride + j], imm_stride 0 shared or D per particle) ;
 *   measure_out[i] = (float)(s_i * (double) acc[i]), rounded once.  A measure that is NaN, +-inf or negative is stored
 *   as exactly 0: a divergent or NaN trial then weighs alpha below and does not poison the sum.  One wavefront per
 *   row; 16-byte accesses when D % 4 == 0 and the arrays are 16-byte aligned.
 * bjx_smc_pretune_weights:  t_i = (double) alpha + (double) measure[i] ; S = sum t ; weights_out[i] = (float)(t_i / S),
 *   uniform 1 / N when S == 0 (alpha 0 and nothing moved).  alpha >= 0 and finite.  One workgroup.
 * bjx_smc_jitter_gather:  out[i, k] = jitter(P[a_i, k], sigma_k, z[a_i, k]), P (N, K), out (M, K), out of place,
 *   a_i = ancestors[i] clamped into [0, N), z = normal(key, (N, K)) (element a_i * K + k: the noise belongs to the
 *   SOURCE row, the reference adds it before it resamples), sigma_k = sigma[k * sigma_stride] (sigma_stride 0: one
 *   scalar, 1: one value per column).  log_space 0: fmaf(sigma, z, p) ; log_space 1: p * exp(sigma * z), the product
 *   and the exponential each rounded to fp32 -- for parameters that must stay positive.  One wavefront per output row,
 *   one thread per row when K == 1.
 * Replaces: smc/pretuning.py::esjd, update_parameter_distribution. */
int bjx_smc_esjd(void* stream, int64_t N, int64_t D, const float* prev, const float* next, const float* acc,
                 const float* imm, int64_t imm_stride, float* measure_out);
int bjx_smc_pretune_weights(void* stream, int64_t N, float alpha, const float* measure, float* weights_out);
int bjx_smc_jitter_gather(void* stream, uint32_t key0, uint32_t key1, int64_t N, int64_t M, int64_t K, const float* P,
                          const int32_t* ancestors, const float* sigma, int64_t sigma_stride, int32_t log_space,
                          float* out);

/* Persistent sampling (blackjax.persistent_sampling_smc / adaptive_persistent_sampling_smc).  Iteration i weighs
 * the P = i * N particles of ALL earlier iterations against the mixture of their tempered targets:
 *   den_j = logsumexp_{s < n_terms}(a_sj - log_Z[s]) - log(n_terms), a_sj = schedule[s] * loglik[j] in fp32 (exactly 0
 *           when schedule[s] == 0, whatever loglik[j] is); the rest in fp64, the maximum subtracted, rounded once
 *   lw_j  = (double)(fp32 *lam * loglik[j]) - (double) den_j ; a NaN or -inf lw_j is a particle of weight 0
 *   lse   = logsumexp_j(lw_j) (fp64) ; *log_Z_out = lse - log P ; weights_out = exp(lw - lse) ;
 *           log_weights_out = lw - lse (-inf for a particle of weight 0).  No particle of positive weight: both
 *           arrays NaN, *log_Z_out = -inf.
 * P reaches 2^24, so the reductions use the whole device: one workgroup per tile of bjx_smc_persistent_tile()
 * particles writes the tile's (max, S1, S2) in fp64 into the workspace and a later launch of one workgroup adds them
 * (launch-separated: no workgroup waits on another).  The tiling depends on P alone, so results are reproducible bit
 * for bit.  workspace: bjx_smc_persistent_workspace_bytes(P) bytes (0 for a P outside [1, 2^24]), 8-byte aligned,
 * contents scratch.  1 <= n_terms ; any of the three outputs of bjx_smc_persistent_weights may be null, not all.
 * Replaces: smc/persistent_sampling.py::compute_log_persistent_weights, compute_log_Z, compute_persistent_weights. */
int bjx_smc_persistent_tile(void);
int64_t bjx_smc_persistent_workspace_bytes(int64_t P);
int bjx_smc_persistent_denominator(void* stream, int64_t P, int64_t n_terms, const float* loglik,
                                   const float* schedule, const float* log_Z, float* den_out);
int bjx_smc_persistent_weights(void* stream, int64_t P, const float* loglik, const float* den, const float* lam,
                               void* workspace, float* log_weights_out, float* weights_out, float* log_Z_out);
/* The next temperature: f(d) = log_ess(lw at lam = *lam_old + d) - log(target), target an ABSOLUTE effective sample
 * size (the caller's N * target_ess; it may exceed N, never P's bound 2^24), log_ess = 2 log S1 - log S2 in fp64.
 *   f(1 - *lam_old) >= 0: delta = 1 - *lam_old and *lam_new_out = 1.0f exactly ; else 30 halvings of [0, 1 - *lam_old]
 *   in fp32, left end moved to mid when f(mid) >= 0, delta = the left end, *lam_new_out = *lam_old + delta.  A target
 *   no temperature reaches gives delta = 0 and *lam_new_out = *lam_old bit for bit.
 * 31 evaluations of f, each a tile launch and a one-workgroup launch that moves the bracket kept in the workspace:
 * 62 launches whatever the data; once the whole interval is taken the remaining ones return at once.
 * Replaces: smc/adaptive_persistent_sampling.py::calculate_lambda ; smc/ess.py::log_ess ; smc/solver.py::dichotomy. */
int bjx_smc_persistent_ess_solve(void* stream, int64_t P, const float* loglik, const float* den, float target,
                                 const float* lam_old, void* workspace, float* delta_out, float* lam_new_out);

/* ---- VI --------------------------------------------------------------------------------------------------------
 * Mean-field variational inference (blackjax.meanfield_vi): a diagonal Gaussian q = N(mu, exp(rho)^2) fitted by
 * stochastic gradient steps on KL(q || p).  The S Monte-Carlo draws of a step are an (S, D) row batch; eps below is
 * normal(key, (S, D)), element (s, d) at flat index s * D + d of the key itself, and sigma_d = exp_cr(rho[d]) (the
 * exponential in fp64, rounded once to fp32).  Every launch is on the caller's stream and reads nothing back.
 * 1 <= S <= 2^24 ; 1 <= D <= 2^20 ; S * D <= 2^31.
 *
 * bjx_vi_meanfield_sample:  z_out[s, d] = fmaf(sigma_d, eps_sd, mu[d]) -- ONE fused multiply-add.  A thread owns
 *   16-byte pieces of the flat (S * D,) array when D % 4 == 0 and mu, rho and z_out are 16-byte aligned, 4-byte
 *   elements otherwise (S may be 5 and D 2^20, so the mapping is flat rather than a wavefront per row).
 * bjx_vi_meanfield_grad:  from G (S, D) and logp (S,), the value and gradient of the target at z, the gradients of
 *   the KL estimate with respect to mu and rho and the estimate itself.  eps is regenerated from the key, so no
 *   (S, D) noise array exists.  Every term is formed in fp64 from the fp32 G, eps and sigma (eps / sigma as eps times
 *   the fp64 reciprocal of sigma), summed in fp64 in a fixed order and rounded once:
 *     stl = 1 (sticking the landing):  g_mu[d] = mean_s(-eps_sd / sigma_d - G_sd)
 *                                      g_rho[d] = mean_s(-eps_sd^2 - G_sd sigma_d eps_sd)
 *     stl = 0:                         g_mu[d] = -mean_s G_sd ;  g_rho[d] = -1 - mean_s(G_sd sigma_d eps_sd)
 *     *kl_out = -(sum_sd eps_sd^2) / (2 S) - sum_d rho[d] - D log(2 pi) / 2 - mean_s logp[s]
 *   Three launches: one workgroup per tile of bjx_vi_meanfield_tile() rows and block of columns (consecutive threads
 *   on consecutive columns) writes the tile's partial sums, one thread per column adds the tiles in order, one
 *   workgroup forms the scalar.  Launch-separated, and the tiling depends on (S, D) alone: the result is reproducible
 *   bit for bit.  A NaN in G[s, d] reaches g_mu[d] and g_rho[d] only.  workspace:
 *   bjx_vi_meanfield_grad_workspace_bytes(S, D) bytes (0 for sizes out of range), 8-byte aligned, contents scratch.
 * Replaces: vi/meanfield_vi.py::sample, step (the Monte-Carlo KL estimate and its jax.value_and_grad). */
int bjx_vi_meanfield_tile(void);
int bjx_vi_meanfield_sample(void* stream, uint32_t key0, uint32_t key1, int64_t S, int64_t D, const float* mu,
                            const float* rho, float* z_out);
int64_t bjx_vi_meanfield_grad_workspace_bytes(int64_t S, int64_t D);
int bjx_vi_meanfield_grad(void* stream, uint32_t key0, uint32_t key1, int64_t S, int64_t D, int32_t stl,
                          const float* G, const float* logp, const float* rho, void* workspace, float* g_mu_out,
                          float* g_rho_out, float* kl_out);
/* Full-rank variational inference (blackjax.fullrank_vi): q = N(mu, L L^T), L lower triangular and packed in
 * chol (D (D + 1) / 2,): chol[i] = log L_ii for i < D, L_ii = exp_cr(chol[i]) (an fp32 value), and
 * L_ij = chol[D + i (i - 1) / 2 + j] for j < i (torch.tril_indices(D, D, -1) order: a row of L is contiguous in j).
 * eps is normal(key, (S, D)) as above.  Every sum below is an fp64 fma chain over the fp32 inputs in a fixed order
 * that depends on (S, D) alone, rounded once to fp32; no atomics, no workgroup waits on another; two calls give
 * identical bits.  The triangle is cut into B x B blocks, B = bjx_vi_fullrank_block(), and the draws into tiles of
 * T = bjx_vi_fullrank_tile() rows.  1 <= S <= 2^20 ; 1 <= D <= 4096 ; S * D <= 2^27.
 *
 * bjx_vi_fullrank_sample:  z_out[s, i] = fp32(mu[i] + sum_{j <= i} L_ij eps_sj), j ascending.  One launch: a
 *   workgroup owns T draws and B columns, regenerates eps a chunk of B columns at a time into LDS and skips the
 *   chunks above the diagonal.
 * bjx_vi_fullrank_grad:  from G (S, D) and logp (S,), with w_s = -u_s - G_s, L^T u_s = eps_s (stl = 1) or
 *   w_s = -G_s (stl = 0), and M = (1 / S) sum_s w_s eps_s^T:
 *     g_mu[i] = mean_s w_si ;  g_chol[D + i (i - 1) / 2 + j] = M_ij (j < i)
 *     g_chol[i] = L_ii M_ii (stl = 1) or -1 + L_ii M_ii (stl = 0)
 *     *kl_out = -(sum_sd eps_sd^2) / (2 S) - sum_{i < D} chol[i] - D log(2 pi) / 2 - mean_s logp[s]
 *   Launches: (stl = 1 only) the solve, a right-looking blocked back-substitution from the last column block to the
 *   first with one launch per column block (workgroup = T draws and one block: the update from the block solved by
 *   the launch before, then, for the next block, u_j = r_j (1 / L_jj) with the fp64 reciprocal and r_i -= L_ji u_j
 *   for i < j), which leaves U in fp64 in the workspace; the outer product, one workgroup per block (I, J <= I) of
 *   the triangle and chunk of draws, w formed from U and G and the eps columns of J regenerated; its combine, which
 *   adds the chunks in order; the column sums of w and eps^2 per tile of bjx_vi_meanfield_tile() rows, their
 *   combine, and the scalar (the mean-field launch).  A NaN in G[s, i] reaches g_mu[i] and row i of the triangle (g_chol[i] and the entries (i, j < i))
 *   only.  workspace: bjx_vi_fullrank_grad_workspace_bytes(S, D) bytes (0 for sizes out of range), 8-byte aligned,
 *   contents scratch; it holds U, so it grows with 8 S D.
 * Replaces: vi/fullrank_vi.py::sample, step (the Monte-Carlo KL estimate and its jax.value_and_grad). */
int bjx_vi_fullrank_tile(void);
int bjx_vi_fullrank_block(void);
int bjx_vi_fullrank_sample(void* stream, uint32_t key0, uint32_t key1, int64_t S, int64_t D, const float* mu,
                           const float* chol, float* z_out);
int64_t bjx_vi_fullrank_grad_workspace_bytes(int64_t S, int64_t D);
int bjx_vi_fullrank_grad(void* stream, uint32_t key0, uint32_t key1, int64_t S, int64_t D, int32_t stl,
                         const float* G, const float* logp, const float* chol, void* workspace, float* g_mu_out,
                         float* g_chol_out, float* kl_out);
/* Element-wise optimiser updates over an (n,) tensor, out of place, mirroring blackjax_amd/optim.py operation by
 * operation in fp32 with no contraction and IEEE division and square root:
 *   adam:  m = (one_minus_b1 * g) + (b1 * mu) ;  v = (one_minus_b2 * (g * g)) + (b2 * nu) ;
 *          u_out = neg_lr * ((m / c1) / (sqrtf(v / c2 + eps_root) + eps)) ;  mu_out = m ;  nu_out = v
 *          c1 = 1 - b1^count and c2 = 1 - b2^count are formed on the host from the host's step count.
 *   sgd:   u_out = neg_lr * g
 * 0 <= n <= 2^31 ; n == 0 is a no-op.
 * Replaces: optax.adam / optax.sgd applied to the (mu, rho) pytree of vi/meanfield_vi.py::step. */
int bjx_optim_adam(void* stream, int64_t n, float b1, float b2, float one_minus_b1, float one_minus_b2, float c1,
                   float c2, float eps, float eps_root, float neg_lr, const float* g, const float* mu, const float* nu,
                   float* mu_out, float* nu_out, float* u_out);
int bjx_optim_sgd(void* stream, int64_t n, float neg_lr, const float* g, float* u_out);

/* Built-in synthetic targets (value + gradient in one pass, fp64-accumulated logp) used
 * as the "user callable" by the bench and parity tests.
 *   diag gaussian:  g = -(q*inv_var) ; logp = 0.5 * sum q*g     (tests/fixtures.py:60-78)
 *   neal funnel:    tests/fixtures.py:81-98
 *   ar1 gaussian:   Sigma_ij = rho^|i-j| (tridiagonal precision)                         */
int bjx_target_diag_gaussian(void* stream, int64_t N, int64_t D, const float* inv_var,
                             const float* q, float* logp_out, float* g_out);
/* The gradient alone, g = -(q*inv_var), bit for bit the g_out of bjx_target_diag_gaussian: what an HMC trajectory
 * with the endpoint proposal needs from every evaluation but its last.  No row reduction, so the launch is one
 * 16-byte piece per lane (D % 4 == 0 and 16-byte aligned buffers; a scalar row loop otherwise). */
int bjx_target_diag_gaussian_grad(void* stream, int64_t N, int64_t D, const float* inv_var,
                                  const float* q, float* g_out);
int bjx_target_neal_funnel(void* stream, int64_t N, int64_t D, const float* q,
                           float* logp_out, float* g_out);
int bjx_target_ar1_gaussian(void* stream, int64_t N, int64_t D, float diag_edge,
                            float diag_mid, float off, const float* q, float* logp_out,
                            float* g_out);

#ifdef __cplusplus
}
#endif

#include "bjx_nuts.h" /* NUTS entry points */

#endif /* BJX_HIP_H */
