/*
 * ocmps.h — C-ABI of the MI355X-native gradient/Hessian inner loop of
 * fskovbo/OptimalControlMPS (BH_tDMRG time-stepper + OptimalControl
 * contractions), implemented by liboptimalcontrolmps_amd.so.
 *
 * Plain pointers and sizes only; no exceptions cross this boundary.  Every
 * function returns 0 on success or a nonzero OCG_E* code, with a message in
 * ocg_last_error(ctx).  The C++ facade (optimalcontrolmps/OptimalControl.hpp)
 * rethrows as std::runtime_error.  Reference citations are path:line in the
 * reference repository.
 *
 * MPS interchange format ("compact U(1) blocks", the IQMPS replacement):
 *   dims : int[(L+1)*(Q+1)]   dims[b*(Q+1)+q] = # states of bond b (between
 *          sites b and b+1; bond 0 and bond L are trivial) whose left particle
 *          count is q.  Q = number of bosons.
 *   data : double[2*nelem]    complex, interleaved (re, im); for site
 *          k = 1..L, sector q = 0..Q, occupation n = 0..p-1 with q+n <= Q and
 *          both dims nonzero: the block A_k[(q,n)] of dims[k-1][q] x
 *          dims[k][q+n] entries, row-major.
 * Every MPS handed in must be right-orthonormal with its orthogonality centre
 * at site 1 (the form BH_tDMRG::step leaves, src/BH_tDMRG.cpp:217-228).
 */
#ifndef OCMPS_H
#define OCMPS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCG_OK 0
#define OCG_EINVAL 1    /* bad argument / shape */
#define OCG_ECAP 2      /* caller buffer too small, or problem exceeds engine capacity */
#define OCG_EHIP 3      /* HIP runtime error (no GPU, launch failure, ...) */
#define OCG_ESTATE 4    /* call order violated (e.g. rows before trajectories) */
#define OCG_ENUM 5      /* numerical failure flagged by a kernel */
#define OCG_ENOMEM 6    /* device or pinned host allocation failed (HBM engine) */

typedef struct ocg_ctx ocg_ctx;

/* Engine limits and per-context sizes (for callers sizing buffers). */
typedef struct ocg_info {
  int L, p, Q;
  size_t mps_max_nelem;   /* complex elements of the largest MPS this context can hold */
  int lds_bytes;          /* dynamic LDS of one chain workgroup */
  int block_threads;      /* threads per chain workgroup */
  int device;
  int fast_chain;         /* 1: every step runs on the one-wave padded chain (LDS engine, small bonds) */
} ocg_info;

/* --------------------------------------------------------------- context
 * Replaces BH_tDMRG(sites, J, tstep, {"Cutoff=",cutoff,"Maxm=",maxm})
 * (reference include/BH_tDMRG.hpp:34, src/BH_tDMRG.cpp:3-15): Bose-Hubbard
 * chain of L sites, local dimension p (= BoseHubbard d + 1), npart bosons,
 * hopping J, Trotter step tstep.  maxm <= 0 means ITensor's default (5000).
 * Builds the forward/backward hopping gates (initJGates, :18-58) and the
 * dH = sum_k 0.5 n_k(n_k-1) MPO data (:10-14) on `device`. */
int ocg_create(int device, int L, int p, int npart, double J, double tstep, double cutoff, int maxm,
               ocg_ctx** out);
/* As ocg_create, choosing the engine: 0 auto (the single-workgroup LDS chain
 * engine when the configuration fits it, else the HBM-resident engine),
 * 1 LDS chain engine only (OCG_ECAP if it does not fit), 2 HBM-resident
 * engine (multi-workgroup, MFMA-FP64 contractions; configurations such as
 * L=20, p=7, chi=256).  Both engines implement every entry point below with
 * the same arithmetic. */
int ocg_create_ex(int device, int L, int p, int npart, double J, double tstep, double cutoff, int maxm, int engine,
                  ocg_ctx** out);
/* number of visible HIP devices (OCG_EHIP and *n = 0 without a GPU) */
int ocg_device_count(int* n);
int ocg_destroy(ocg_ctx* ctx);
/* last error message of ctx (or of the last failed ocg_create when ctx == NULL) */
const char* ocg_last_error(const ocg_ctx* ctx);
/* writes sizeof(ocg_info) bytes of the header the library was built with
 * (since ABI version 3: fast_chain is the last field); callers built against
 * another version use ocg_get_info_sz */
int ocg_get_info(const ocg_ctx* ctx, ocg_info* info);
/* as ocg_get_info, writing at most info_size bytes (the caller's sizeof(ocg_info)) */
int ocg_get_info_sz(const ocg_ctx* ctx, ocg_info* info, size_t info_size);
/* ABI version of the library (OCG_ABI_VERSION of the header it was built with).
 * Changelog: 2 ocg_info.fast_chain (round 5), OCG_ENOMEM returned by
 * ocg_hessian when OCG_HBM_PIPE=1 forces a pipeline that cannot allocate;
 * 3 ocg_get_info_sz, ocg_get_path_stats, ocg_abi_version (round 6);
 * 4 ocg_observe, ocg_observe_states, ocg_kernel_stats kind 9;
 * 5 ocg_observe_spectrum, ocg_observe_spectrum_states;
 * 6 ocg_sample, ocg_sample_states, ocg_fock_amplitudes, ocg_fock_amplitudes_states;
 * 7 ocg_observe_moments, ocg_observe_moments_states; added within 7 (no existing
 * entry point or struct changed): ocg_observe_pairs, ocg_observe_pairs_states;
 * ocg_observe_strings, ocg_observe_strings_states; ocg_set_potential,
 * ocg_get_potential. */
#define OCG_ABI_VERSION 7
int ocg_abi_version(void);
/* BH_tDMRG::setTstep (src/BH_tDMRG.cpp:61-65) */
int ocg_set_tstep(ocg_ctx* ctx, double tstep);

/* Static site potential sum_k eps_k n_k (trap, tilt, superlattice, disorder;
 * DESIGN.md §15).  eps points to L doubles (site 1 first) or is NULL to clear
 * it; all zeros is the same as NULL.  NaN / inf: OCG_EINVAL.  It applies to
 * every later call that steps a state, in real and in imaginary time, on both
 * engines: one step from u_from to u_to over tau = +-tstep is
 * D_to G_odd G_even D_from with D_x = prod_k exp(-i tau [u_x n_k (n_k - 1) / 4
 * + eps_k n_k / 2]).  dH/dU is unchanged.  Setting it drops the device
 * trajectories like ocg_set_tstep.  ocg_get_potential writes L doubles (zeros
 * when none is set).  (Additions within ABI version 7.) */
int ocg_set_potential(ocg_ctx* ctx, const double* eps);
int ocg_get_potential(const ocg_ctx* ctx, double* eps);
/* number of complex elements of an MPS with the given dims */
size_t ocg_mps_nelem(int L, int p, int Q, const int* dims);

/* ------------------------------------------ TimeStepper-level operations
 * Host MPS in, host MPS out (compact format above).  out_cap is the capacity
 * of out_data in complex elements; *out_nelem receives the size written.
 * Input dims are checked on the host before anything reaches the device, on
 * both engines (these calls, ocg_step_batch, ocg_overlap, ocg_apply_dH,
 * ocg_set_states): a negative entry, or a bond 0 / bond L that is not the one
 * state q = 0 / q = Q, OCG_EINVAL; a sector above its Schmidt-rank bound
 * min(HS_left, HS_right) OCG_ECAP. */

/* BH_tDMRG::step(psi, from, to, propagateForward) (src/BH_tDMRG.cpp:111-230) */
int ocg_step(ocg_ctx* ctx, const int* dims, const double* data, double from, double to, int forward,
             int* out_dims, double* out_data, size_t out_cap, size_t* out_nelem);
/* nsteps consecutive steps with controls u[0..nsteps] (step i: u[i] -> u[i+1]) */
int ocg_steps(ocg_ctx* ctx, const int* dims, const double* data, const double* u, int nsteps, int forward,
              int* out_dims, double* out_data, size_t out_cap, size_t* out_nelem);
/* Batched BH_tDMRG::step over n independent states, one device launch
 * (SURVEY.md §8b `ocg_step_batch`): state i = (dims + i*(L+1)*(Q+1), data[i])
 * takes one step u_from[i] -> u_to[i] in direction `forward`; the result goes
 * to (out_dims + i*(L+1)*(Q+1), out_data[i]) of capacity out_cap[i] complex
 * elements, size in out_nelem[i].  Uses scratch slots after the trajectories
 * (device psi_t / xi_t / xiH_t are left intact). */
int ocg_step_batch(ocg_ctx* ctx, int n, const int* dims, const double* const* data, const double* u_from,
                   const double* u_to, int forward, int* out_dims, double* const* out_data, const size_t* out_cap,
                   size_t* out_nelem);
/* Ground-state preparation on the device (replaces ITensor DMRG in
 * InitializeState, include/InitializeState.hpp:18-117): nsteps imaginary-time
 * Trotter steps exp(-tau H_BH(J, U)) of the state, the sweep of
 * BH_tDMRG::step with exp(-tau h) gates and exp(-tau U n(n-1)/4) phases,
 * normalised, truncated with the context's Cutoff/Maxm.  The context's
 * real-time gates and device trajectories are left as they were.  The C++
 * facade's InitializeState runs a tau schedule over this. */
int ocg_imag_steps(ocg_ctx* ctx, const int* dims, const double* data, double U, double tau, int nsteps,
                   int* out_dims, double* out_data, size_t out_cap, size_t* out_nelem);
/* InitializeState's ground state (include/InitializeState.hpp:18-117) in one
 * call with the state resident on the device: for each tau of taus[0..ntau),
 * imaginary-time steps (as ocg_imag_steps) in blocks of `block` until
 * 1 - |<state before the block|state after>| < tol or max_steps per stage; one
 * device overlap per block, no host round trip.  Returns the final state;
 * *steps_done (optional) = total steps taken.  Real-time gates and device
 * trajectories are left as they were. */
int ocg_ground_state(ocg_ctx* ctx, const int* dims, const double* data, double U, int ntau, const double* taus,
                     int block, double tol, int max_steps, int* out_dims, double* out_data, size_t out_cap,
                     size_t* out_nelem, int* steps_done);
/* overlapC(x, y) = <x|y> (with_dH = 0) or overlapC(x, propDeriv, y) = <x|dH|y>
 * (with_dH = 1) (src/OptimalControl.cpp:242, :412); out = {re, im} */
int ocg_overlap(ocg_ctx* ctx, const int* dims_x, const double* x, const int* dims_y, const double* y,
                int with_dH, double* out);
/* exactApplyMPO(propDeriv, psi, args) (src/OptimalControl.cpp:256); *norm = ||result|| */
int ocg_apply_dH(ocg_ctx* ctx, const int* dims, const double* data, int* out_dims, double* out_data,
                 size_t out_cap, size_t* out_nelem, double* norm);

/* ----------------------------------------- OptimalControl hot path
 * Device-resident trajectories for one control vector u[0..N-1].
 * OptimalControl ctor copies of psi_target / psi_init (src/OptimalControl.cpp:10-34). */
int ocg_set_states(ocg_ctx* ctx, const int* dims_target, const double* target, const int* dims_init,
                   const double* init);
/* calcPsi (which & 1, src/OptimalControl.cpp:375-390) and calcXi (which & 2,
 * :392-407); both chains run concurrently when which == 3 (calcPsiXiDivT's
 * two threads, :421-438). */
int ocg_propagate(ocg_ctx* ctx, const double* u, int N, int which);
/* overlapFactor = overlapC(psi_t[N-1], psi_target) (src/OptimalControl.cpp:242) */
int ocg_overlap_factor(ocg_ctx* ctx, double* F);
/* fid[i] = |<psi_target|psi_t[i]>|^2 (calcFidelityForAllT, :548-569) */
int ocg_fidelities(ocg_ctx* ctx, double* fid);
/* divT[i] = overlapC(xi_t[i], propDeriv, psi_t[i]) (calcDivT, :409-419); 2N doubles */
int ocg_div_t(ocg_ctx* ctx, double* divT);
/* xiHlist[i] = exactApplyMPO(propDeriv, xi_t[i], args) for all i (:300-303) */
int ocg_xi_dH(ocg_ctx* ctx);
/* calcHessianRow (:251-279) for rows[0..nrows-1] (each in 1..N-2), F and divT
 * as produced above (F: 2 doubles, divT: 2N doubles).  Writes the fidelity
 * Hessian entries (i, j>=i) and their mirrors into H (row-major N x N,
 * caller-zeroed; entries of different rows are disjoint); the regularisation
 * Hessian is the caller's.  Requires ocg_propagate(..,3) + ocg_xi_dH. */
int ocg_hessian_rows(ocg_ctx* ctx, const double* u, int N, const int* rows, int nrows, const double* F,
                     const double* divT, double* H);
/* One full getHessian(u, new_control = true) fidelity part, fused
 * (calcHessian_parallel, src/OptimalControl.cpp:281-338, without the
 * regularisation Hessian, which is the caller's): psi_t and xi_t, xiHlist,
 * divT, F and the rows[0..nrows-1] (each in 1..N-2).  Rows start as soon as
 * their psi_i is available and the <xiH_j|psiH> overlaps run as one batched
 * launch afterwards; arithmetic per row is that of ocg_hessian_rows.  H is
 * row-major N x N, caller-zeroed (rows' entries and mirrors written); divT
 * (2N doubles) and F (2) are returned for the gradient.  Leaves the same
 * device state as ocg_propagate(..,3) + ocg_xi_dH. */
int ocg_hessian(ocg_ctx* ctx, const double* u, int N, const int* rows, int nrows, double* H, double* divT,
                double* F);
/* K control vectors u[k*N .. k*N+N) in one call (IPOPT line-search trial
 * points, finite-difference probes, multi-start; no reference counterpart: the
 * reference evaluates one getHessian at a time, src/OptimalControl.cpp:281-338).
 * LDS engine: one k_pipeline launch carries all K controls' psi / xi chains,
 * xiH workers and rows (tickets keep every waiter behind its producers), then
 * one batched divT / F launch and one row-overlap launch; per control exactly
 * the arithmetic of ocg_hessian (the same H bit for bit).  HBM engine: the
 * controls in turn.  H: K row-major N x N blocks, caller-zeroed; divT: K x 2N;
 * F: K x 2.  Leaves control 0's trajectories as ocg_hessian would. */
int ocg_hessian_multi(ocg_ctx* ctx, int K, const double* u, int N, const int* rows, int nrows, double* H,
                      double* divT, double* F);
/* getAnalyticGradient's device work for one control vector (calcPsi || calcXi,
 * calcDivT and F = <psi_{N-1}|psi_target>, src/OptimalControl.cpp:204-249,
 * :375-419): divT (2N doubles, complex) and F (2 doubles).  = ocg_propagate(..,3)
 * + ocg_div_t + ocg_overlap_factor, whose trajectories it leaves on the device,
 * unless the HBM engine's stored trajectories would not fit half the free HBM
 * (config 5 at N_t = 1001): then psi and xi run as one lockstep batch that
 * meets in the middle (psi_0..psi_{N/2} and xi_{N/2+1}..xi_{N-1} stored, the
 * other halves paired as they are produced): N states instead of 2N, the same
 * N-1 dependent steps, the same numbers bit for bit, no trajectories left
 * (OCG_HBM_MID=1 / 0 forces either path). */
int ocg_gradient(ocg_ctx* ctx, const double* u, int N, double* divT, double* F);
/* The gradient's device work (calcPsi || calcXi + divT + F, the BFGS path of
 * calcFidelityGrad, src/OptimalControl.cpp:204-249) for K control vectors
 * u[k*N .. k*N+N) in one call: LDS engine, one trajectory launch of 2K chains
 * and one batched divT / F launch each (per control exactly the arithmetic of
 * ocg_propagate(..,3) + ocg_div_t + ocg_overlap_factor); HBM engine, one
 * lockstep batch of 2K chains + one batched divT / F overlap launch each when
 * the grown state heap (the context's slots + 2N per extra control) fits half
 * the free HBM (the extra slots are released afterwards), else — or when the
 * batched call fails to allocate — the controls in turn.  Either way the same
 * numbers bit for bit.  divT: K x 2N, F: K x 2; grad_k,i = dt Re(i divT_k,i F_k)
 * (plus the caller's regularisation).  Leaves control 0's trajectories. */
int ocg_gradient_multi(ocg_ctx* ctx, int K, const double* u, int N, double* divT, double* F);
/* which: 0 psi_t, 1 xi_t, 2 xiHlist; copy trajectory state t to the host.
 * Gauge: the chains skip doStep's closing position(1) (src/BH_tDMRG.cpp:206-218)
 * on every step but their last, so an intermediate psi_t / xi_t is the same
 * state with its orthogonality centre on the last gate's left site (site 2 for
 * L >= 3) instead of site 1; the final states (psi_{N-1}, xi_0) and everything
 * ocg_steps returns are in the reference's gauge. */
int ocg_get_state(ocg_ctx* ctx, int which, int t, int* dims, double* data, size_t cap, size_t* nelem);

/* Observables of the device-resident trajectory states, evaluated where the
 * states are (the drivers' loops over OC.getPsit(): <N_i>, <N_i^2>, bond
 * dimensions, a+a / nn correlation rows).  which: 0 psi_t, 1 xi_t, 2 xiHlist,
 * existing as for ocg_get_state (OCG_ESTATE otherwise).  ts[0..nt): state
 * indices in 0..N-1, any order, repeats allowed; ts == NULL: 0..nt-1.
 * rows[0..nrows): start sites in 1..L (nrows == 0: no correlations).
 * Outputs (NULL: skipped, and its work not done):
 *   norm2[nt]                 <s|s>
 *   occ[nt][L][p]             raw occupation distribution (not divided by
 *                             norm2): <N> = sum n occ, <NN> = sum n^2 occ, ...
 *   bond[nt][L+1]             bond dimensions
 *   corr_ada[nt][nrows][L][2] <a+_i a_j> for j >= i, interleaved (re, im)
 *   corr_nn[nt][nrows][L]     <n_i n_j> for j >= i
 * Entries j < i of a row are 0 (rho_ji = conj(rho_ij)); the j = i entries are
 * real (sum n occ, sum n^2 occ).  Gauge-free (environments from both ends), so
 * intermediate, unnormalised and truncated states are fine.  The states are
 * processed in chunks whose workspace fits half the free device memory
 * (OCG_ENOMEM if not even one state's does); a state's results are bit-identical
 * whatever else is requested with it.  Reads the trajectories only. */
int ocg_observe(ocg_ctx* ctx, int which, const int* ts, int nt, const int* rows, int nrows, double* norm2,
                double* occ, int* bond, double* corr_ada, double* corr_nn);
/* The same for n caller-supplied host states (state i = dims + i*(L+1)*(Q+1),
 * data[i]; any gauge or norm), staged in the scratch slots behind the
 * trajectories as ocg_step_batch does, in batches. */
int ocg_observe_states(ocg_ctx* ctx, int n, const int* dims, const double* const* data, const int* rows, int nrows,
                       double* norm2, double* occ, int* bond, double* corr_ada, double* corr_nn);

/* Entanglement (Schmidt) spectra and entropies of the device-resident
 * trajectory states at every bond b = 1..L-1 (between sites b and b+1):
 * AnalyzeQuench's entanglementEntropy(sites, psi) (include/correlations.hpp:
 * 119-149) evaluated where the states are.  which, ts and the existence rules
 * are those of ocg_observe.  With Lenv / Renv the environments of ocg_observe
 * (Lenv_k[q'] = sum A^H Lenv_{k-1} A, Renv_{k-1}[q] = sum A Renv_k A^H) the
 * weights of bond b in sector q (left particle count) are the eigenvalues of
 * X = S^H Renv_b[q] S, S = V diag(sqrt(max(lambda, 0))), Lenv_b[q] = V
 * diag(lambda) V^H: gauge-free, raw (their sum over a bond is norm2).  A
 * sector of dims without an Lenv or Renv block contributes dims[b][q] zero
 * weights, so a bond always has bond[b] weights.
 * Outputs (NULL: skipped):
 *   entropy[nt][L-1]        S_b = -sum_{p > 1e-12} p ln p over p = max(w, 0) /
 *                           sum max(w, 0) (natural log; 0 for a zero state)
 *   schmidt[nt][L-1][wcap]  the weights of the bond, descending, ties by sector
 *                           ascending; entries past the bond dimension are 0
 *   sector[nt][L-1][wcap]   the sector q of each weight; -1 past the bond dimension
 * wcap below a requested state's largest bond dimension: OCG_ECAP when schmidt
 * or sector is wanted (ignored otherwise).  Bond sectors of order up to 512
 * (OCG_ECAP above); OCG_ENUM if a Jacobi eigen block does not converge.
 * Chunked as ocg_observe; a state's results are bit-identical whatever else is
 * requested with it.  Only results leave the device (the weights only when
 * asked for).  Reads the trajectories only. */
int ocg_observe_spectrum(ocg_ctx* ctx, int which, const int* ts, int nt, int wcap, double* entropy,
                         double* schmidt, int* sector);
/* The same for n caller-supplied host states (as ocg_observe_states: any gauge
 * or norm; a sector may be larger than its Schmidt-rank bound), staged on the
 * device in batches. */
int ocg_observe_spectrum_states(ocg_ctx* ctx, int n, const int* dims, const double* const* data, int wcap,
                                double* entropy, double* schmidt, int* sector);

/* Projective occupation snapshots of the device-resident trajectory states: nshots
 * samples n = (n_1 .. n_L) per state drawn from |<n|s>|^2 / <s|s> (what a
 * quantum-gas microscope records), drawn where the states are.  which, ts and the
 * existence rules are those of ocg_observe; any gauge and any norm.  With A_k(q, n)
 * the blocks and Renv the right environments of ocg_observe (Renv_L[Q] = 1) a shot
 * runs left to right from v = [1], q = 0; at site k = 1..L
 *   w_n  = v A_k(q, n)                                  (a row vector)
 *   pr_n = max(Re(w_n Renv_k[q+n] w_n^H), 0)            (0 without a block or Renv)
 *   c_n  = pr_0 + .. + pr_n (added in that order), S = c_{p-1}
 * and the draw is the smallest n with u S < c_n (if rounding leaves none, the
 * largest n with pr_n > 0); then v = w_n, q += n.  Nothing is renormalised on the
 * way.  logp = ln |v|^2 - ln norm2 with the final 1 x 1 v and norm2 = the S of
 * site 1 (= Renv_0[0] = <s|s>).  A shot that meets S == 0 (a zero state) has -1 at
 * every site and logp = -inf; that is no error.
 * Random numbers are counter-based: with mix the splitmix64 step
 *   x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *   x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^= x >> 31
 * h = mix(mix(mix(mix(seed) ^ id) ^ shot) ^ k), u = (h >> 11) * 2^-53, id = ts[e]
 * (the state index; the position i for ocg_sample_states), shot = 0..nshots-1,
 * k = 1..L.  So the same t requested twice gives the same shots, the first m
 * shots of a larger request are those of a request of m, and which is not mixed
 * in (vary the seed).  A shot is bit-identical whatever else is requested with it
 * and however the request is chunked.
 * Outputs: config[nt][nshots][L] occupations; logp[nt][nshots] (NULL: skipped).
 * nshots < 0: OCG_EINVAL; nshots == 0 writes nothing.  Bond sectors of order up
 * to 512 (OCG_ECAP above).  Chunked as ocg_observe (OCG_ENOMEM if one state's
 * workspace does not fit); only the results leave the device.  Reads the
 * trajectories only. */
int ocg_sample(ocg_ctx* ctx, int which, const int* ts, int nt, int nshots, unsigned long long seed,
               signed char* config, double* logp);
/* The same for n caller-supplied host states (as ocg_observe_spectrum_states: any
 * gauge or norm; a sector may be larger than its Schmidt-rank bound), staged on the
 * device in batches; id = the position of the state in the call. */
int ocg_sample_states(ocg_ctx* ctx, int n, const int* dims, const double* const* data, int nshots,
                      unsigned long long seed, signed char* config, double* logp);
/* Amplitudes <n|s> of given configurations: the chain v -> v A_k(q, n_k) of
 * ocg_sample with the n given and no Renv (no right sweep), amp = the final 1 x 1
 * v; 0 when the path meets a missing block.  Raw: the sum of |amp|^2 over all
 * configurations is norm2.  configs[nconf][L]; an entry outside 0..p-1 or a
 * configuration that does not hold Q particles: OCG_EINVAL.
 * amp[nt][nconf][2], interleaved (re, im).  nconf == 0 writes nothing. */
int ocg_fock_amplitudes(ocg_ctx* ctx, int which, const int* ts, int nt, const signed char* configs, int nconf,
                        double* amp);
int ocg_fock_amplitudes_states(ocg_ctx* ctx, int n, const int* dims, const double* const* data,
                               const signed char* configs, int nconf, double* amp);

/* Energy moments of stored states.  With H(J, U) = -J K + U D,
 * K = sum_{i<L} (a+_i a_{i+1} + a_i a+_{i+1}) (a, a+ cut at p levels, as the
 * gates) and D = sum_i n_i (n_i - 1) / 2 (the dH of the context), state s gives
 *   mom[7] = { norm2 = <s|s>, k1 = <s|K|s>, d1 = <s|D|s>, kk = <s|K K|s>,
 *              dd = <s|D D|s>, kd_re, kd_im = <s|K D|s> }
 * raw (none divided by norm2) and independent of J and U, so that for any (J, U)
 *   E = (-J k1 + U d1) / norm2,
 *   Var = (J^2 kk - 2 J U kd_re + U^2 dd) / norm2 - E^2,
 *   d<D>/dt = -2 J kd_im / norm2 (hbar = 1).
 * A left-to-right sweep of the environments of the operator automaton (0 nothing
 * yet, 1 a+ placed, 2 a placed, 3 a K term done, 4 a D term done) for the left and
 * the right operator of each product: no right environments, so the centre may sit
 * anywhere and the state need not be normalised.  A state without a surviving path
 * gives zeros.  which / ts / existence rules and chunking as ocg_observe
 * (OCG_ENOMEM if one state's workspace exceeds the chunk budget); bond sectors of
 * order up to 512 (OCG_ECAP above).  States whose sectors are all at most 16 wide
 * (in a context with Q <= 244) run in one kernel per chunk (OCG_OBS_ENERGY_CHAIN=0: the task-list path for
 * all; the two agree to rounding, not bit for bit).  A state's numbers depend on
 * the state and its path alone: bit-identical whatever else is requested and
 * however the request is chunked.  mom[nt][7]; nt == 0 writes nothing.  Reads the
 * trajectories only. */
int ocg_observe_moments(ocg_ctx* ctx, int which, const int* ts, int nt, double* mom);
/* The same for n caller-supplied host states (as ocg_observe_spectrum_states: any
 * gauge or norm, zero-padded sectors allowed), staged on the device in batches. */
int ocg_observe_moments_states(ocg_ctx* ctx, int n, const int* dims, const double* const* data, double* mom);

/* Transition matrix elements between two stored states.  Pair e has the bra x (state
 * tx[e] of trajectory which_x) and the ket y (state ty[e] of which_y); which 0 psi_t,
 * 1 xi_t, 2 xiH_t, existence rules, OCG_ESTATE / OCG_EINVAL as ocg_observe; tx == NULL
 * or ty == NULL means 0..npairs-1; npairs == 0 writes nothing.  The outputs are
 * complex, interleaved (re, im) and raw (nothing is divided by a norm); a NULL output
 * is skipped and its work is not done:
 *   ovl[npairs][2]            <x|y>
 *   occ[npairs][L][p][2]      <x|P_k(n)|y>, P_k(n) the projector on occupation n of site
 *                             k: <x|n_k|y> = sum_n n occ, <x|D|y> = sum_k sum_n n (n - 1) / 2 occ
 *   hop[npairs][L-1][2][2]    [b-1][0] = <x|a+_b a_{b+1}|y>, [b-1][1] = <x|a_b a+_{b+1}|y>
 *                             (a, a+ cut at p levels, as the gates); <x|K|y> = the sum of
 *                             both over b.
 * Gauge free, environments from both ends as ocg_observe; they are rectangular (block
 * q is d_x[b][q] x d_y[b][q]), so x and y may have different bond dimensions, and a
 * sector only one of them has contributes nothing.  Any norm.  Chunking and
 * OCG_OBS_BUDGET as ocg_observe_moments (OCG_ENOMEM if one pair's workspace exceeds the
 * chunk budget); bond sectors of order up to 512 (OCG_ECAP above).  Pairs whose sectors
 * are all at most 16 wide, both states, run in one kernel per chunk (OCG_OBS_PAIR_CHAIN=0:
 * the task-list path for all, 5 L - 2 launches per chunk, 2 L + 1 for ovl alone; the two
 * agree to rounding, not bit for bit).  A pair's numbers depend on the pair and its
 * path alone: bit-identical whatever else is requested, in whatever order, and however
 * the request is chunked.  Reads the trajectories only.  Counted in ocg_kernel_stats
 * kind 9. */
int ocg_observe_pairs(ocg_ctx* ctx, int which_x, const int* tx, int which_y, const int* ty, int npairs, double* ovl,
                      double* occ, double* hop);
/* The same for n pairs of caller-supplied host states (x[e], y[e]; any gauge or norm,
 * zero-padded sectors allowed), staged on the device in batches. */
int ocg_observe_pairs_states(ocg_ctx* ctx, int n, const int* dims_x, const double* const* x, const int* dims_y,
                             const double* const* y, double* ovl, double* occ, double* hop);

/* Expectations of products of diagonal one-site operators (string operators) in stored
 * states: parity (string) order, the counting statistics of a block, multi-point
 * projector correlators.  f[nops][L][p][2] are complex tables, interleaved (re, im);
 * operator m is O_m = (x)_k F_{m,k} with F_{m,k} = sum_n f[m][k-1][n] P_k(n), P_k(n) the
 * projector on occupation n of site k (the projector of ocg_observe_pairs).
 *   out[nt][nops][2] = <s|O_m|s>, complex, raw (not divided by <s|s>), gauge free, any norm.
 * which, ts (NULL: 0..nt-1; repeats and any order are fine), existence rules and
 * OCG_ESTATE / OCG_EINVAL as ocg_observe.  nops == 0 or nt == 0 writes nothing.
 * OCG_EINVAL: nops < 0, f == NULL with nops > 0, a table entry that is not finite.
 *
 * The numbers.  The support [a, b] of operator m runs from its first to its last site
 * whose table is not exactly (1, 0) for every n.  With an empty support out = norm2.
 * Otherwise, with Lenv / Renv the environments of ocg_observe and A_k(q, n) block (q, n)
 * of site k,
 *   E_{a-1}[q] = Lenv_{a-1}[q]
 *   E_k[q+n]  += f[k][n] A_k(q,n)^H E_{k-1}[q] A_k(q,n)        k = a..b
 *   out        = sum_q sum E_b[q] o Renv_b[q]^T                 (= sum_q tr(E_b[q] Renv_b[q])).
 * A block that does not exist contributes nothing: the level cut (p - 1 < Q), empty
 * sectors, sectors of dims with no block.  The work per operator is proportional to its
 * support length, not to L; Lenv and Renv are formed once per state, however many
 * operators there are.
 *
 * Bond sectors of order up to 512 (OCG_ECAP above).  Chunking and OCG_OBS_BUDGET as
 * ocg_observe_moments (OCG_ENOMEM if the workspace of one state with all its operators
 * exceeds the chunk budget).  States whose sectors are all at most 16 wide run in two
 * kernels per chunk, whatever nops and nt are (OCG_OBS_STRING_CHAIN=0: the task-list path
 * for all, 2 (L - 1) + 2 M + 1 launches per chunk with M the longest support, an empty
 * one counting 1; the two paths agree to rounding, not bit for bit).  <s|O_m|s> depends
 * on s, on table m and on the path alone: bit-identical whatever other operators or
 * states are requested, in whatever order, and however the request is chunked.  Reads
 * the trajectories only.  Counted in ocg_kernel_stats kind 9. */
int ocg_observe_strings(ocg_ctx* ctx, int which, const int* ts, int nt, const double* f, int nops, double* out);
/* The same for n caller-supplied host states (any gauge or norm, zero-padded sectors
 * allowed), staged on the device in batches as ocg_observe_pairs_states. */
int ocg_observe_strings_states(ocg_ctx* ctx, int n, const int* dims, const double* const* data, const double* f,
                               int nops, double* out);

/* ControlBasis::convertHessian (src/ControlBasis.cpp:91-116) on the device:
 * Hc (M x M) = V Hu V^T with Hu row-major N x N (host), V row-major M x N
 * (V[n][i] = S_i f_{i n}, the transposed control Jacobian).  Each entry is a
 * sequential inner product in the reference's order without fused
 * multiply-adds: bit-identical to the host restatement.  Any engine. */
int ocg_convert_hessian(ocg_ctx* ctx, const double* Hu, int N, const double* V, int M, double* Hc);

/* ITensor denmatDecomp(M, A, B, Fromleft, {"Cutoff=",cutoff,"Maxm=",maxm})
 * (called at src/BH_tDMRG.cpp:178, :191, :209) of nm independent dense
 * blocks M[i] (rows[i] x cols[i] complex, row-major, 0 < rows <= cols <= any,
 * rows <= 512), each one U(1) sector: the decomposition every two-site update
 * of the HBM engine runs (Gram M M^H, Hermitian eigensolver, truncation rule,
 * eigenvectors, factors), on caller-supplied matrices, batched in one pass.
 * kept[i] = k; A[i] (rows x k, orthonormal columns) and B[i] = A^H M (k x
 * cols), both row-major complex, caller buffers of rows*rows / rows*cols
 * complex elements (NULL: not returned); w[i] (rows doubles, NULL: not
 * returned) = the Gram eigenvalues as the eigensolver leaves them (order not
 * specified; those below ~1e-3 cutoff / rows of the trace may be unresolved).
 * HBM engine contexts only (ocg_create_ex engine 2); else OCG_EINVAL. */
int ocg_denmat_decomp(ocg_ctx* ctx, int nm, const int* rows, const int* cols, const double* const* M,
                      double cutoff, int maxm, int* kept, double* const* w, double* const* A, double* const* B);

/* ------------------------------------------------------ instrumentation
 * Per-kernel HIP-event timing on the context's stream and the algorithmic
 * traffic model of DESIGN.md §Roofline.  kind: 0 trajectory, 1 overlaps,
 * 2 dH apply, 3 Hessian rows, 4 steps, 5 fused pipeline (ocg_hessian phase 1),
 * 6 batched row overlaps (ocg_hessian phase 2), 7 the HBM engine's MFMA GEMM
 * kernel (k_gemm: HIP-event time, algorithmic bytes and flops of its tasks;
 * zeros on the LDS engine), 8 the HBM engine's getHessian path counters
 * (*launches = pipelined getHessians completed, *sweep_steps = two-phase
 * retries after a pipeline that failed with OCG_ENOMEM; never with
 * OCG_HBM_PIPE=1, which makes any pipeline failure the call's status),
 * *alg_flops = trajectory-checkpointed getHessians completed, *alg_bytes = the
 * segment length of the last one), 9 the observable kernels of ocg_observe /
 * ocg_observe_states / ocg_observe_spectrum[_states] / ocg_sample[_states] /
 * ocg_fock_amplitudes[_states] / ocg_observe_moments[_states] / ocg_observe_pairs[_states] /
 * ocg_observe_strings[_states] (HIP-event time of their chunks, kernel launches, and the
 * algorithmic bytes and flops of the host-built task lists).  Sums since the
 * last reset. */
int ocg_kernel_stats(ocg_ctx* ctx, int kind, double* total_ms, long* launches, double* alg_bytes,
                     double* alg_flops, long* sweep_steps);
int ocg_reset_stats(ocg_ctx* ctx);
/* Which paths the HBM engine's calls took since the context was created (named
 * counters; ocg_kernel_stats kind 8 returns the first four through its timing
 * fields and stays for old callers).  The caller sets out->size =
 * sizeof(ocg_path_stats); only that many bytes are written.  Zeros on the LDS
 * engine. */
typedef struct ocg_path_stats {
  size_t size;           /* set by the caller: sizeof(ocg_path_stats) of its header */
  long pipe_runs;        /* pipelined getHessians completed */
  long pipe_fallbacks;   /* two-phase reruns after a pipeline that failed with OCG_ENOMEM */
  long ckpt_runs;        /* trajectory-checkpointed getHessians completed */
  long ckpt_k;           /* segment length of the last checkpointed getHessian */
  long coop_launches;    /* multi-CU eigenvalue launches (k_heev_vals_coop) */
  long coop_groups;      /* Gram blocks reduced by a group of workgroups */
  long coop_fallbacks;   /* of those, groups that gave up a wait and were re-run on one CU */
} ocg_path_stats;
int ocg_get_path_stats(ocg_ctx* ctx, ocg_path_stats* out);
/* diagnostic builds (-DOCG_PROFILE) only: shader-clock cycles per engine phase
 * (32 slots, see engine_device.hpp Chain::pf), summed over workgroups; zeros in
 * the product build.  reset != 0 clears after reading. */
int ocg_profile(ocg_ctx* ctx, double* out32, int reset);

#ifdef __cplusplus
}
#endif
#endif /* OCMPS_H */
