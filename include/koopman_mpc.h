/*
 * koopman_mpc.h — C ABI of the batched Koopman-MPC controller.
 *
 * The reference runs one Koopman-MPC controller on one env, serially, with casadi/IPOPT
 * (control/MPC_Controler.py) inside the Koopman_MPC.py tracking loop:
 *
 *   MPCController.Psi_o(s)        z = [x, MLP(x)] lifted state       control/MPC_Controler.py:154-167
 *                                 (Koopmanlinear.x_encoder, models/KoopmanBase.py:45-47)
 *   MPCController.setup_delta_mpc unconstrained QP over H = 10 moves   control/MPC_Controler.py:100-141
 *   MPCController.setup_mpc       (the same over absolute inputs)      control/MPC_Controler.py:65-98
 *   MPCController.get_control(p)  u0 = u_opt[0] + u_prev, a = clip    control/MPC_Controler.py:143-152
 *   Test.runMPC                   lifted refs, z0, solve, env.step     Koopman_MPC.py:197-222
 *
 * The QP has no constraints (nlpsol is called without bounds, MPC_Controler.py:145) and a
 * constant Hessian for the linear Koopman model (DKUC, the default), so IPOPT's optimum is the
 * closed form  u0 = Gr·r + Gz·z0 + Gu·u_prev  (r = the H lifted reference points stacked).
 * The host computes (Gr, Gz, Gu) once per controller; these entry points run the per-env work
 * on the GPU for a whole batch of envs:
 *
 *   sim_koopman_encode       Psi_o for M states (f64 MFMA encoder)
 *   sim_koopman_feedforward  Gr·r for every frame of a reference trajectory (f64 MFMA)
 *   sim_koopman_mpc_step     z0 = Psi_o(x); u0; a = clip(u0); u_prev = u0 (one launch)
 *   sim_koopman_box_step     the DKUC step with input limits: a box QP per env (ADMM on the f64 MFMA)
 *   sim_koopman_bilinear_box_step  the same for the bilinear DBKN model: a box QP with its own Hessian
 *                            per env and frame (projected Gauss-Seidel in registers, one wave per env)
 *   sim_koopman_predict      the model's multi-step open-loop prediction of recorded trajectories
 *                            and its error (evaluate(), train.py:35-87; one launch for all steps)
 *   sim_koopman_train_step   one training step of the DKUC model: loss, gradient and Adam in two
 *                            launches (train(), train.py:89-266; k_linear_loss, models/losses.py:54-129)
 *
 * Arithmetic is float64 throughout, as in the reference (model.double(), Koopman_MPC.py:263).
 * Device buffers are caller-owned; calls are asynchronous on the given stream (void* =
 * hipStream_t, NULL = default).  Errors: negative SIM_E_* codes (soarm_sim.h) and
 * sim_last_error().
 */
#ifndef KOOPMAN_MPC_H
#define KOOPMAN_MPC_H

#include <stdint.h>

#include "soarm_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_KMAXLAYER 6 /* encoder linear layers */
#define SIM_KMAXW 64    /* hidden / output width of every encoder layer */
#define SIM_KMAXX 8     /* x_dim */
#define SIM_KMAXU 8     /* u_dim */
#define SIM_KMAXH 32    /* horizon */

typedef struct sim_koopman_desc {
  int32_t x_dim;                    /* 8: [ee_xyz(3), q(5)] (args.x_dim)  */
  int32_t u_dim;                    /* 5 (args.u_dim) */
  int32_t nlayer;                   /* linear layers of x_encode_net (5 for args.layers) */
  int32_t width[SIM_KMAXLAYER + 1]; /* [x_dim, 64, 64, 64, 64, 24] (args.py:103) */
  int32_t horizon;                  /* H = 10 (MPC_Controler.py:27) */
  int32_t _pad;
  double u_clip;                    /* 0.5: a = clip(u0, -0.5, 0.5) (MPC_Controler.py:149) */
} sim_koopman_desc;

typedef struct sim_koopman sim_koopman;

/* weights: per layer l, W_l [width[l+1]][width[l]] row-major (nn.Linear.weight) then b_l
   [width[l+1]]; ReLU between layers, none after the last (models/KoopmanBase.py:20-25).
   gain: [u_dim][H*nz + nz + u_dim] row-major = [Gr | Gz | Gu], nz = x_dim + width[nlayer]. */
int sim_koopman_create(const sim_koopman_desc* desc, const double* weights, const double* gain,
                       int device, sim_koopman** out);
void sim_koopman_free(sim_koopman* k);

/* Psi_o: z [nz][m] (SoA) = [x, MLP(x)] for x [m][x_dim] float32 rows (the reference lifts
   DoubleTensor(obs), obs being float32, Koopman_MPC.py:220-221). */
int sim_koopman_encode(sim_koopman* k, int m, const float* x, double* z, void* stream);

/* Feedforward of a lifted reference trajectory: for frame f < nframe,
   ff[f][u][e] = sum_t Gr_t · zref[f + 1 + t][:][e], terms with f + 1 + t >= nref being zero
   (the reference pads the window past the trajectory end with zero rows, Koopman_MPC.py:199-205).
   zref [nref][nz][n], ff [nframe][u_dim][n]. */
int sim_koopman_feedforward(sim_koopman* k, int nframe, int nref, int n, const double* zref, double* ff,
                            void* stream);

/* One control step for n envs: z0 = Psi_o(x) (or the given z0 [nz][n]), then
   u0 = ff + Gz z0 + Gu u_prev; u_prev <- u0; action = clip(u0) as float32.
   x [n][x_dim] float32 (ignored when z0 != NULL), ff [u_dim][n] (NULL = 0),
   u_prev [u_dim][n] in/out, action [n][u_dim]. */
int sim_koopman_mpc_step(sim_koopman* k, int n, const float* x, const double* z0, const double* ff,
                         double* u_prev, float* action, void* stream);

/* The bilinear DBKN model (models/KoopmanBase.py:62-110): its input matrix is linearised at each
   env's lifted state, B_total = B + sum_j z0_j Hhat_j (linearize_B, MPC_Controler.py:46-63), so
   the condensed QP of MPC_Controler.py:65-141 (state_full: Q = q I, R = r I) is solved per env and
   frame.  set_bilinear: A [nz][nz], B [nz][u_dim], Hhat [nz (j)][nz][u_dim] (get_Hi_numpy), delta
   (1 = 'delta_mpc', 0 = 'mpc'), q = 50, r = 0.5.  bilinear_step: z0 [nz][n], window [H][nz][n]
   (lifted reference rows k+1 .. k+H, zero past the end), u_prev [u_dim][n] in/out (u_prev <- u0),
   action [n][u_dim] = clip(u0) float32.  Replaces the casadi solve of get_control for DBKN. */
int sim_koopman_set_bilinear(sim_koopman* k, const double* A, const double* B, const double* Hhat, int delta,
                             double q, double r);
int sim_koopman_bilinear_step(sim_koopman* k, int n, const double* z0, const double* window, double* u_prev,
                              float* action, void* stream);

/* The DKUC control step with input limits (csrc/koopman_box.hip).  sim_koopman_mpc_step solves the
   unconstrained horizon QP and clips its first move; the plan it optimised never knew the limit.
   This step minimises the same cost (MPC_Controler.py:80-86 / :115-127, state_full: q = 50, r = 0.5)
   over plans whose every model input, and the input that is applied, stays in [-u_max, u_max].
   In the model inputs w [N = H u_dim]:
     'delta_mpc' (delta != 0)  w_t = u_prev + sum_{i<=t} du_i, |w_t| <= u_max, u0 = w_0;
     'mpc'                     w_t = v_t, |v_t| <= u_max for t >= 1 and |v_0 + u_prev| <= u_max
                               (the reference applies u_opt[0] + u_prev, :147), u0 = v_0 + u_prev;
   both are  min 1/2 w'Pw - g'w,  lo <= w <= hi,  P = P(A, B, H, kind, q, r) the same for every env
   and frame, g affine in (window, z0, u_prev).

   set_box (host, once per model; independent of set_bilinear / set_model): builds P, Lhat = ||P||_inf,
   P's extreme eigenvalues, the gains of the unconstrained minimiser wu = P^-1 g and the ADMM step
   matrix rho (P + rho I)^-1, rho = sqrt(lambda_min lambda_max), as MFMA fragments, and uploads them.
   opts NULL = the defaults (u_max = the controller's u_clip, tol 1e-9, max_iter 256).
   SIM_E_MODEL (with the limit in the message): N > 64, nz > 64, an LDS plan over 160 KiB.
   SIM_E_ARG: NULL k / A / B, u_max <= 0, tol <= 0, max_iter < 1, q or r <= 0, a bad struct header.
   A refusal leaves every other entry point working and box_step refused.
   sim_koopman_box_check (an entry point beside the two above, so that the refusals can be asked for
   without a device or a handle) runs the same option and shape checks as set_box -- one pair of
   helpers serves both -- from the desc alone; it returns SIM_OK or the code set_box would return for
   them.  set_box first drops the state of an earlier set_box, then runs those checks.

   box_step, n envs: z0 = Psi_o(x) unless z0 [nz][n] is given; window [H][nz][n] the lifted reference
   rows k+1 .. k+H (zero past the end); u_prev [u_dim][n] in/out (u_prev <- u0); action [n][u_dim] =
   (float)u0 (no clip: u0 is in the box); plan [H][u_dim][n] or NULL: on return the model inputs w_t;
   warm != 0 with a plan: the plan as given (the caller passes last frame's, shifted or not) is a
   candidate start beside the cold one, clip(wu): the iteration starts from clip(plan) where
   res(clip(plan)) < res(clip(wu)) mu / (4 Lhat) or <= tol, i.e. where the plan is provably the closer of the two
   (res / 2 <= ||w - w*|| <= 2 (Lhat / mu) res), else cold; ok [n], iters [n] int32 or NULL.
   Stop test: with res(w) = w - clip(w - (P w - g) / Lhat, lo, hi) an env is done when ||res(w)||_inf <=
   tol: ok = 1, iters = the iterations it took.  An env whose wu lies in the box returns it with iters =
   0, warm or not, and a wave whose 16 envs all do leaves before the iteration (the matrices of the
   iteration are not even staged when that holds for the whole workgroup).  An env that reaches
   max_iter gets ok = 0, iters = max_iter and its last iterate, which is a projection: inside the box.
   Deterministic; an env's result does not depend on n or on its neighbours (columns of an MFMA).
   No allocation, copy or synchronisation: capturable in a graph.
   SIM_E_ARG before any launch: set_box not called (or refused), NULL k / window / u_prev / action,
   n < 0, x and z0 both NULL.  n == 0 is a no-op. */
typedef struct sim_koopman_box_opts {
  int32_t struct_size; /* sizeof(sim_koopman_box_opts) */
  int32_t abi_version; /* SIM_ABI_VERSION */
  int32_t max_iter;    /* 256 (twice the measured maximum, rounded up) */
  int32_t _pad;
  double u_max;        /* 0.5 */
  double tol;          /* 1e-9 */
} sim_koopman_box_opts;

int sim_koopman_box_check(const sim_koopman_desc* desc, const sim_koopman_box_opts* opts);
int sim_koopman_set_box(sim_koopman* k, const double* A, const double* B, int delta, double q, double r,
                        const sim_koopman_box_opts* opts);
int sim_koopman_box_step(sim_koopman* k, int n, const float* x, const double* z0, const double* window,
                         double* u_prev, double* plan, int warm, float* action, int32_t* ok, int32_t* iters,
                         void* stream);

/* The DBKN control step with input limits (csrc/koopman_bilinear.hip, k_bilinear_box): the problem of
   sim_koopman_box_step above -- the same kinds, bounds and u0 -- with B_total = B + sum_j z0_j Hhat_j
   in place of B, so P = P_e differs per env and frame and nothing of it can be prepared on the host.
   One wave per env builds P_e as sim_koopman_bilinear_step builds its Hessian and solves the box QP by
   projected Gauss-Seidel in registers, from w = clip(0), in the order of the time blocks from the last
   to the first.  There is no factorisation: an env whose unconstrained minimiser lies inside the box
   is iterated like every other (iters > 0, solved to tol), unlike box_step's iters = 0.

   set_bilinear_box runs after sim_koopman_set_bilinear and takes that call's A, B, Hhat, kind, q and
   r; opts NULL = the defaults (u_max = the controller's u_clip, tol 1e-9, max_iter 128: DESIGN.md
   section 5, twice the measured maximum of 61 sweeps, rounded up).
   SIM_E_ARG: NULL k, set_bilinear not called, u_max <= 0, tol <= 0, max_iter < 1, a bad struct header.
   The kernel runs on bilinear_step's LDS plan and on fewer registers, so every shape set_bilinear
   accepts is accepted (no SIM_E_MODEL of its own).  A refusal leaves bilinear_box_step refused and
   every other entry point working; a later set_bilinear drops the box state.

   bilinear_box_step, n envs: z0 [nz][n], window [H][nz][n], u_prev [u_dim][n] in/out (u_prev <- u0) as
   bilinear_step; action [n][u_dim] = (float)u0 (no clip: u0 is in the box); plan [H][u_dim][n] or
   NULL: on return the model inputs w_t in natural order ('mpc': v_t); ok [n], iters [n] int32 or NULL.
   Stop test, after every sweep: res(w) = w - clip(w - (P_e w - g_e) / Lhat_e, lo, hi), Lhat_e =
   ||P_e||_inf; done when ||res||_inf <= tol: ok = 1, iters = the sweeps it took (>= 1).  An env that
   reaches max_iter gets ok = 0, iters = max_iter and its last iterate, which is a projection: inside
   the box.  There is no warm start.  Deterministic; an env's result does not depend on n or on its
   neighbours (one wave per env).  No allocation, copy or synchronisation: capturable in a graph.
   SIM_E_ARG before any launch: set_bilinear_box not called (or refused), NULL k / z0 / window /
   u_prev / action, n < 0.  n == 0 is a no-op. */
int sim_koopman_set_bilinear_box(sim_koopman* k, const sim_koopman_box_opts* opts);
int sim_koopman_bilinear_box_step(sim_koopman* k, int n, const double* z0, const double* window,
                                  double* u_prev, double* plan, float* action,
                                  int32_t* ok, int32_t* iters, void* stream);

/* Open-loop prediction and its error: how well the Koopman model predicts recorded trajectories.
   This is what evaluate() (train.py:35-87) reports, through pred_and_eval_loss_old
   (models/losses.py:132-173); relift = 0 is the latent rollout of pred_and_eval_loss_new
   (models/losses.py:175-215).  One launch runs all T steps of n trajectories; the lifted state
   stays in registers.

   set_model: A [nz][nz], B [nz][u_dim]; Hhat [nz (j)][nz][u_dim] for DBKN (the array of
   sim_koopman_set_bilinear, get_Hi_numpy: the u_z permutation is already in it) or NULL for DKUC.
   Independent of sim_koopman_set_bilinear.  SIM_E_MODEL when the encoder and the model do not fit
   the kernel's LDS plan (sim_koopman_predict then returns SIM_E_MODEL too).

   predict: rows [T+1][n][ld] float32 row-major, x at columns x_off .. x_off + x_dim, u at
   u_off .. u_off + u_dim (a rollout of the data generator, [u(5) | ee(3) | q(5)], is read in place
   with ld = 13, x_off = 5, u_off = 0).  Float64 from the widened float32 inputs.  Per trajectory e:
     x^_0 = x_0, z = Psi(x_0);
     t = 0 .. T-1:  z <- A z + (B + sum_j z_j Hhat_j) u_t;  x^_{t+1} = z[:x_dim] (the reference's
                    frozen decoder lC = [I | 0]);  relift != 0:  z <- Psi(x^_{t+1}).
   pred [T+1][n][x_dim] (row 0 = x_0), or NULL.
   err [2][n], or NULL: err[0][e] = sum_t sum_{d < npos} |x^_{t+1,d} - x_{t+1,d}|, err[1][e] the same
   over d >= npos; deterministic (per-trajectory sums in a fixed order, no atomics).  The reference's
   pred_loss / dis_loss / angle_loss are global means of these sums (npos = 3).
   SIM_E_ARG: NULL k or rows, n < 0, T < 0, npos outside 0 .. x_dim, columns past ld, set_model not
   called.  n == 0 is a no-op.  No allocation, copy or synchronisation: capturable in a graph. */
int sim_koopman_set_model(sim_koopman* k, const double* A, const double* B, const double* Hhat);
int sim_koopman_predict(sim_koopman* k, int n, int T, const float* rows, int ld, int x_off, int u_off,
                        int relift, int npos, double* pred, double* err, void* stream);

/* Training (train(), train.py:89-266, with k_linear_loss, models/losses.py:54-129, loss_name "mse"):
   one step of the DKUC model's fit is two launches -- the loss and its gradient, then the reduction
   and Adam -- with no host synchronisation.  (loss_name "nmse" and "weighted_mse": set_loss, below.)

   The trainer owns, on one device: the parameter vector (float64), Adam's m and v, the step count of
   the bias correction, the MFMA-fragment copies the kernels read and a per-wave partial-gradient
   workspace for max_batch windows.  The parameter vector, sim_koopman_trainer_nparam doubles, no
   padding:  [W_0 | b_0 | ... | W_{nl-1} | b_{nl-1} | A (nz x nz row-major) | B (nz x u_dim row-major)]
   -- the `weights` of sim_koopman_create, then the A and B of sim_koopman_set_model.  The decoder
   lC = [I | 0] is frozen (models/KoopmanBase.py:38-43) and is no parameter.

   Loss of n windows starting at row t0, P = pre_length, Psi(x) = [x, MLP(x)], beta_i = gamma^i,
   cont = sum_i beta_i:   z^_0 = Psi(x_t0);  i < P:  z^_{i+1} = A z^_i + B u_{t0+i},
     koopman = sum_i beta_i mean_{n nz}    (z^_{i+1} - Psi(x_{t0+i+1}))^2 / cont
     pred    = sum_i beta_i mean_{n x_dim} (z^_{i+1}[:x_dim] - x_{t0+i+1})^2 / cont
     dis / angle: pred over the columns < npos / >= npos, each with its own mean
     recon   = 0 (lC Psi(x) = x exactly);   total = koopman + pred + recon.
   The gradient is that of `total` with respect to the parameter vector (the two regularisers
   k_linear_loss computes but leaves out of total_loss, losses.py:116-118, are not built).

   opts: struct_size / abi_version as the other by-pointer structs; pre_length 1..64; npos
   1..x_dim-1; gamma > 0; Adam's beta1, beta2, eps (torch.optim.Adam, no weight decay).
   create: SIM_E_MODEL for a shape the kernels do not cover (nlayer > 5, LDS), SIM_E_NODEVICE
   without a GPU; desc.horizon and desc.u_clip are validated as by sim_koopman_create and unused.
   get_params / set_params: synchronous host copies; reset_optimizer != 0 zeroes m, v and the step count.

   loss_grad / train_step: rows [T+1][N][ld] float32 as sim_koopman_predict reads them (x at x_off,
   u at u_off; widened to float64); traj_idx [n] int32 on the device picks the window's trajectory
   (repeats allowed; values are clamped to 0..N-1) or NULL for trajectories 0..n-1; t0 the window's
   first row.  losses [6] device doubles (total, koopman, pred, recon, dis, angle) or NULL; grad
   [nparam] device doubles or NULL.  loss_grad changes no trainer state.  train_step then applies
       m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;
       p <- p - lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps),   t = steps so far + 1
   to the parameter vector and every fragment copy.  Partial gradients are summed in a fixed order
   (no floating-point atomics): results are bitwise reproducible.  Neither call allocates, copies
   between host and device or synchronises.
   SIM_E_ARG before any launch: NULL tr or rows, n < 0, n > max_batch, N < 1, n > N with traj_idx
   NULL, t0 < 0, t0 + pre_length > T, columns past ld.  n == 0 is a no-op.

   The bilinear DBKN model (models/KoopmanBase.py:62-78; the same train() and k_linear_loss):
   sim_koopman_trainer_create_bilinear makes a trainer of the same handle type whose step is
       z^_{i+1} = A z^_i + B u_{t0+i} + H vec(z^_i (x) u_{t0+i})      (u_z = 0)
                                      + H vec(u_{t0+i} (x) z^_i)      (u_z = 1)
   with everything else -- the losses, the encoder, Adam, the calls above, their refusals -- as for
   DKUC.  Its parameter vector is DKUC's followed by one block, sim_koopman_trainer_nparam_bilinear =
   sim_koopman_trainer_nparam + nz nz u_dim doubles:
       [... | A | B | H (nz x nz u_dim row-major)],
   H exactly as net.H.weight in the net's own u_z order: column j u_dim + c multiplies z_j u_c for
   u_z = 0, column c nz + j for u_z = 1 (sim_koopman_set_bilinear's Hhat is H with that permutation
   undone).  With H_c (nz x nz) the block of H that multiplies u_c z, the step is A z + B u + sum_c
   H_c (u_c z), its adjoint dH_c += lambda_{i+1} (u_c z^_i)' and lambda_i = g_i + A' lambda_{i+1} +
   sum_c u_c H_c' lambda_{i+1}; u is data and has no gradient.  The sparsity and spectral-radius terms
   of H that k_linear_loss computes but leaves out of total_loss are not built either.
   create_bilinear: SIM_E_ARG for u_z other than 0 or 1; every other refusal as create's.

   The loss (k_linear_loss's loss_name, BaseLoss, models/losses.py:35-52) is a property of the trainer:
   a new one is SIM_KLOSS_MSE, the loss above; sim_koopman_trainer_set_loss selects how later
   loss_grad / train_step calls launch and touches nothing else (not the parameters, Adam's state or the
   step count; no allocation: the workspace of every loss is made by create).  Both other losses apply
   BaseLoss to the same four pairs -- koopman (z^, Psi(x)), pred, dis, angle -- per step, combined with
   beta_i / cont as above; recon stays exactly 0 with a zero gradient.  With e = z^_{i+1} - Psi(x_{t0+i+1}),
   ex its x columns:
     SIM_KLOSS_NMSE  mse(preds, labels) / mean(labels^2) = sum (preds - labels)^2 / sum labels^2 over the
       whole minibatch: koopman_i = sum e^2 / sum Psi(x)^2, pred_i = sum ex^2 / sum x^2, dis / angle the same
       over their columns.  The label is not detached in the reference: koopman's normaliser depends on the
       encoder and carries a gradient, which the step includes.  A zero normaliser gives inf or NaN as in
       torch; it is not guarded.  The normalisers must precede every backward, so this step is four
       launches (the sums, their reduction, then the two above).
     SIM_KLOSS_WEIGHTED_MSE  (mse(first three columns) + 9 mse(the other columns)) / 10; the split at column
       3 is the reference's literal constant, not npos, and needs x_dim >= 4.  dis and angle split their own
       slice at its column 3: a slice of three columns or fewer has no "other columns", the reference's
       value is then NaN (the mean of an empty tensor) and so is this one -- dis with the default npos = 3,
       angle with x_dim - npos <= 3.  They are logged, not trained: total and the gradient stay finite.
   The reference's fourth name, mae, is its evaluation metric (sim_koopman_predict), not a training choice
   of args.py, and is not built.
   set_loss: SIM_E_ARG for a NULL tr, an unknown id, or SIM_KLOSS_WEIGHTED_MSE with x_dim < 4; the trainer
   then keeps its loss.  get_loss: the id, or SIM_E_ARG for NULL. */
#define SIM_KLOSS_MSE 0
#define SIM_KLOSS_NMSE 1
#define SIM_KLOSS_WEIGHTED_MSE 2

typedef struct sim_koopman_train_opts {
  int32_t struct_size; /* sizeof(sim_koopman_train_opts) */
  int32_t abi_version; /* SIM_ABI_VERSION */
  int32_t pre_length;  /* 5 */
  int32_t npos;        /* 3: the dis / angle split of x */
  double gamma;        /* 0.8 (args.py:68) */
  double beta1;        /* 0.9 */
  double beta2;        /* 0.999 */
  double eps;          /* 1e-8 */
} sim_koopman_train_opts;

typedef struct sim_koopman_trainer sim_koopman_trainer;

int sim_koopman_trainer_nparam(const sim_koopman_desc* desc);
int sim_koopman_trainer_create(const sim_koopman_desc* desc, const double* params, int max_batch,
                               const sim_koopman_train_opts* opts, int device, sim_koopman_trainer** out);
int sim_koopman_trainer_nparam_bilinear(const sim_koopman_desc* desc);
int sim_koopman_trainer_create_bilinear(const sim_koopman_desc* desc, const double* params, int u_z, int max_batch,
                                        const sim_koopman_train_opts* opts, int device, sim_koopman_trainer** out);
void sim_koopman_trainer_free(sim_koopman_trainer* tr);
int sim_koopman_trainer_set_loss(sim_koopman_trainer* tr, int loss);
int sim_koopman_trainer_get_loss(const sim_koopman_trainer* tr);
int sim_koopman_trainer_get_params(sim_koopman_trainer* tr, double* host_params);
int sim_koopman_trainer_set_params(sim_koopman_trainer* tr, const double* host_params, int reset_optimizer);
int sim_koopman_loss_grad(sim_koopman_trainer* tr, int n, int N, int T, const float* rows, int ld, int x_off,
                          int u_off, const int32_t* traj_idx, int t0, double* losses, double* grad, void* stream);
int sim_koopman_train_step(sim_koopman_trainer* tr, int n, int N, int T, const float* rows, int ld, int x_off,
                           int u_off, const int32_t* traj_idx, int t0, double lr, double* losses, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_MPC_H */
