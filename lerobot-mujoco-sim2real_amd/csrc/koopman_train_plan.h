// koopman_train_plan.h — the host-side plan of the Koopman trainer (koopman_train.hip): where every
// parameter sits in the plain vector, where its copies sit in the MFMA-fragment blob the kernels
// read, the workspace sizes, and the argument checks of the per-step calls.  Plain C++ (no HIP),
// so tools/koopman_train_selftest.cpp runs it under the host sanitizers without a GPU.
//
// Parameter vector (sim_koopman_trainer_nparam doubles, no padding):
//   [W_0 | b_0 | ... | W_{nl-1} | b_{nl-1} | A (nz x nz row-major) | B (nz x u_dim row-major)]
// Fragment blob (doubles; every fragment is 64 lanes: lane l holds M[16 T + (l & 15)][4 s + (l >> 4)]
// of output tile T and k-step s):
//   encoder   W_l [ntile][ks][64] and the biases [nl][64], in KDev's layout (staged into LDS);
//   wt[l]     W_l' for l >= 1: [4 (input tiles)][4 ntile[l]][64] (the backward's W' delta);
//   ab        [A | B]: [1 + ntl][2 + 4 ntl + 2][64], tile 0 = the x rows, tiles 1.. = the features,
//             k order [x (8) | features (16 ntl) | u (8)] (k_predict's);
//   at        A': [1 + ntl][2 + 4 ntl][64] over the same tile and k orders.
// The bilinear plan (DBKN, make_plan(..., bil = true, u_z)) appends one block to each of the three:
//   parameters  H (nz x nz u_dim row-major, net.H.weight in the net's own u_z order) after B;
//   blob        hf [u_dim][1 + ntl][2 + 4 ntl][64]: H_c in the tile and k order of the A part of ab,
//               right after at; then ht, H_c' in at's order.  H_c (nz x nz) is the block of H that
//               multiplies u_c z: H_c[i][j] = H[i][c nz + j] (u_z = 1) or H[i][j u_dim + c] (u_z = 0)
//               -- the order is a matter of the index map alone;
//   slot        sH: dH_c as [u_dim][1 + ntl][1 + ntl] tiles in the C/D layout, right after [dA | dB].
// The kernel derives the three offsets from at, sA and the shape, so the DKUC plan's numbers and the
// kernels' argument struct are what they were.
#ifndef KOOPMAN_TRAIN_PLAN_H
#define KOOPMAN_TRAIN_PLAN_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/koopman_mpc.h"
#include "koopman_layout.h"

namespace ktrain {

constexpr int MAXL = 5;         // encoder layers the wave's scratch plan covers (4 hidden x 64 rows)
constexpr int MAXP = 64;        // pre_length
constexpr int TILE_LD = 18;     // doubles per row of a wave's 16 x 16 transpose tile (see k_koopman_grad)
constexpr int WAVES = 4;        // waves per workgroup
constexpr size_t LDS_BYTES = KOOPMAN_LDS_BYTES;

struct Plan {
  int xd, ud, nl, outw, nz, ntl, P, npos;
  int width[SIM_KMAXLAYER + 1];
  int ntile[SIM_KMAXLAYER], ks[SIM_KMAXLAYER], frag[SIM_KMAXLAYER];  // encoder (klayout::Encoder's)
  int bias, enc_total;                                             // doubles staged in LDS
  int wt[SIM_KMAXLAYER], kst[SIM_KMAXLAYER];                       // W_l' fragments, their k-steps
  int ab, abks, at, atks;
  int bil, uz;  // the bilinear plan (DBKN) and its H column order; hf, ht, pH, sH are -1 without it
  int hf, ht;   // H_c, H_c' fragments: [ud][1 + ntl][atks][64] each
  int blob_total;
  int pw[SIM_KMAXLAYER], pb[SIM_KMAXLAYER], pA, pB, pH, nparam;  // offsets into the parameter vector
  // a wave's partial-gradient slot: every product's output tiles in the C/D layout, [tile][r][64]
  // (lane l, register r = row (l >> 4) + 4 r, column l & 15 of the tile)
  int sw[SIM_KMAXLAYER];  // dW_l: [ntile[l]][input tiles: 1 (l = 0) or 4]
  int sb[SIM_KMAXLAYER];  // db_l: [64]
  int sA;                 // [dA | dB]: [1 + ntl][1 + ntl + 1], the last tile column = dB
  int sH;                 // dH_c: [ud][1 + ntl][1 + ntl]
  int slot_stride;   // doubles of a slot: the above + 8 (the loss sums)
  int scr_stride;    // doubles of one wave's scratch: z^ and g [P][2][1 + ntl][4][64], then one
                     // encode's hidden activations [MAXL - 1][4][4][64]
  size_t lds_bytes;  // dynamic LDS of k_koopman_grad
};

// the shape checks of sim_koopman_create, then the trainer's own; fills pl.  SIM_OK or an error
// code with its message in err
inline int make_plan(const sim_koopman_desc& d, const sim_koopman_train_opts& o, Plan& pl, std::string& err,
                     bool bil = false, int u_z = 0) {
  if (int rc = klayout::check_desc(d, err)) return rc;
  const int xd = d.x_dim, ud = d.u_dim, nl = d.nlayer;
  if (nl > MAXL)
    return err = "trainer: nlayer must be <= 5 (the scratch plan keeps four hidden layers' activations)",
           SIM_E_MODEL;
  if (o.pre_length < 1 || o.pre_length > MAXP) return err = "trainer: pre_length must be in 1..64", SIM_E_ARG;
  if (o.npos < 1 || o.npos >= xd) return err = "trainer: npos must be in 1..x_dim-1 (dis and angle are means)", SIM_E_ARG;
  if (!(o.gamma > 0.0)) return err = "trainer: gamma must be positive", SIM_E_ARG;
  if (!(o.beta1 >= 0.0 && o.beta1 < 1.0) || !(o.beta2 >= 0.0 && o.beta2 < 1.0) || !(o.eps >= 0.0))
    return err = "trainer: beta1, beta2 must be in [0, 1) and eps >= 0", SIM_E_ARG;
  if (bil && u_z != 0 && u_z != 1) return err = "trainer: u_z must be 0 (vec(z (x) u)) or 1 (vec(u (x) z))", SIM_E_ARG;
  pl = Plan{};
  pl.bil = bil, pl.uz = bil ? u_z : 0, pl.hf = pl.ht = pl.pH = pl.sH = -1;
  pl.xd = xd, pl.ud = ud, pl.nl = nl, pl.outw = d.width[nl], pl.nz = xd + d.width[nl];
  pl.P = o.pre_length, pl.npos = o.npos;
  for (int l = 0; l <= nl; l++) pl.width[l] = d.width[l];
  const klayout::Encoder enc = klayout::encoder(d);
  for (int l = 0; l < nl; l++) pl.ntile[l] = enc.ntile[l], pl.ks[l] = enc.ks[l], pl.frag[l] = enc.frag[l];
  pl.ntl = enc.ntl, pl.bias = enc.bias, pl.enc_total = enc.total;
  int off = enc.total;
  for (int l = 1; l < nl; l++) {
    pl.kst[l] = 4 * pl.ntile[l];
    pl.wt[l] = off;
    off += 4 * pl.kst[l] * 64;
  }
  pl.abks = klayout::ks_zu(enc), pl.atks = klayout::ks_z(enc);
  pl.ab = off, off += (1 + pl.ntl) * pl.abks * 64;
  pl.at = off, off += (1 + pl.ntl) * pl.atks * 64;
  if (bil) {
    pl.hf = off, off += ud * (1 + pl.ntl) * pl.atks * 64;
    pl.ht = off, off += ud * (1 + pl.ntl) * pl.atks * 64;
  }
  pl.blob_total = off;
  int p = 0;
  for (int l = 0; l < nl; l++) {
    pl.pw[l] = p, p += d.width[l + 1] * d.width[l];
    pl.pb[l] = p, p += d.width[l + 1];
  }
  pl.pA = p, p += pl.nz * pl.nz;
  pl.pB = p, p += pl.nz * ud;
  if (bil) pl.pH = p, p += pl.nz * pl.nz * ud;
  pl.nparam = p;
  int so = 0;
  for (int l = 0; l < nl; l++) {
    pl.sw[l] = so, so += pl.ntile[l] * (l == 0 ? 1 : 4) * 256;
    pl.sb[l] = so, so += 64;
  }
  pl.sA = so, so += (1 + pl.ntl) * (2 + pl.ntl) * 256;
  if (bil) pl.sH = so, so += ud * (1 + pl.ntl) * (1 + pl.ntl) * 256;
  pl.slot_stride = so + 8;
  pl.scr_stride = pl.P * 2 * (1 + pl.ntl) * 4 * 64 + (MAXL - 1) * 4 * 4 * 64;
  pl.lds_bytes = ((size_t)pl.enc_total + (size_t)WAVES * 16 * TILE_LD) * sizeof(double);
  if (pl.lds_bytes > LDS_BYTES)
    return err = "trainer: the encoder fragments and the transpose tiles (" + std::to_string(pl.lds_bytes) +
                 " bytes) do not fit the 160 KiB of LDS",
           SIM_E_MODEL;
  return SIM_OK;
}

// the nmse loss's workspace: the waves' per-step sums [max_slot][P][8] doubles (k_koopman_stats), and the
// table k_koopman_nmse_table makes of them -- [P][4] per-step coefficients, then 8 doubles for the six
// losses.  The table shares the step count's buffer, STEP_DOUBLES doubles in (the count is one int): the
// gradient and apply kernels find it from the pointer they already take, so their argument lists do
// not depend on the loss
constexpr int STEP_DOUBLES = 1;
inline size_t stat_doubles(const Plan& pl, int max_slot) { return (size_t)max_slot * pl.P * 8; }
inline size_t tab_doubles(const Plan& pl) { return (size_t)pl.P * 4 + 8; }
inline size_t step_bytes(const Plan& pl) { return (STEP_DOUBLES + tab_doubles(pl)) * sizeof(double); }

// the padded row and k maps (klayout::z_of_row, z_of_k, u_of_k) read these fields of the plan
inline klayout::Encoder layout_of(const Plan& pl) {
  klayout::Encoder e{};
  e.xd = pl.xd, e.ud = pl.ud, e.nl = pl.nl, e.outw = pl.outw, e.nz = pl.nz, e.ntl = pl.ntl;
  return e;
}

// parameter index of H_c[i][j] (bilinear plan)
inline int h_param(const Plan& pl, int c, int i, int j) {
  return pl.pH + i * (pl.nz * pl.ud) + (pl.uz ? c * pl.nz + j : j * pl.ud + c);
}

// map[c][p], c = 0, 1: the blob positions parameter p is copied to (-1 = none).  Every parameter has
// one or two; false if a position is claimed twice or a parameter has none or more than two
inline bool index_map(const Plan& pl, std::vector<int32_t>& map) {
  map.assign((size_t)2 * pl.nparam, -1);
  std::vector<uint8_t> used((size_t)pl.blob_total, 0);
  bool ok = true;
  auto put = [&](int p, int pos) {
    if (p < 0 || p >= pl.nparam || pos < 0 || pos >= pl.blob_total || used[pos]) {
      ok = false;
      return;
    }
    used[pos] = 1;
    if (map[p] < 0)
      map[p] = pos;
    else if (map[(size_t)pl.nparam + p] < 0)
      map[(size_t)pl.nparam + p] = pos;
    else
      ok = false;
  };
  using klayout::each_frag;
  const klayout::Encoder e = layout_of(pl);
  auto zrow = [&](int row) { return klayout::z_of_row(e, row >> 4, row & 15); };
  for (int l = 0; l < pl.nl; l++) {
    const int in = pl.width[l], ou = pl.width[l + 1];
    each_frag(pl.ntile[l], pl.ks[l], [&](int pos, int row, int col) {
      if (row < ou && col < in) put(pl.pw[l] + row * in + col, pl.frag[l] + pos);
    });
    for (int r = 0; r < ou; r++) put(pl.pb[l] + r, pl.bias + l * SIM_KMAXW + r);
    if (l >= 1)  // W_l': rows = the layer's inputs, k = its outputs
      each_frag(4, pl.kst[l], [&](int pos, int row, int k) {
        if (row < in && k < ou) put(pl.pw[l] + k * in + row, pl.wt[l] + pos);
      });
  }
  for (int tile = 0; tile <= pl.ntl; tile++) {  // (tile by tile: the order decides which copy is map[0])
    each_frag(1, pl.abks, [&](int pos, int r, int kk) {
      const int i = klayout::z_of_row(e, tile, r), j = klayout::z_of_k(e, kk), c = klayout::u_of_k(e, kk);
      if (i >= 0 && j >= 0) put(pl.pA + i * pl.nz + j, pl.ab + tile * pl.abks * 64 + pos);
      if (i >= 0 && c >= 0) put(pl.pB + i * pl.ud + c, pl.ab + tile * pl.abks * 64 + pos);
    });
    each_frag(1, pl.atks, [&](int pos, int r, int kk) {
      const int j = klayout::z_of_row(e, tile, r), i = klayout::z_of_k(e, kk);
      if (i >= 0 && j >= 0) put(pl.pA + i * pl.nz + j, pl.at + tile * pl.atks * 64 + pos);
    });
  }
  if (pl.bil)  // H_c as A's part of ab, H_c' as at: every H parameter has exactly these two copies
    for (int c = 0; c < pl.ud; c++)
      each_frag(1 + pl.ntl, pl.atks, [&](int pos, int row, int kk) {
        const int r = zrow(row), k = klayout::z_of_k(e, kk);
        if (r < 0 || k < 0) return;
        const int o = c * (1 + pl.ntl) * pl.atks * 64 + pos;
        put(h_param(pl, c, r, k), pl.hf + o);
        put(h_param(pl, c, k, r), pl.ht + o);
      });
  for (int p = 0; p < pl.nparam; p++)
    if (map[p] < 0) ok = false;
  return ok;
}

// position in a tile-ordered slot region (nti tile columns) of element (row, col)
inline int slot_pos(int base, int nti, int row, int col) {
  const int Tr = row >> 4, Tc = col >> 4, rr = row & 15, cc = col & 15;
  return base + ((Tr * nti + Tc) * 4 + (rr >> 2)) * 64 + (rr & 3) * 16 + cc;
}
// padded row / column of lifted-state index z in the [x (16) | features] tile space
inline int z_pad(const Plan& pl, int z) { return z < pl.xd ? z : 16 + (z - pl.xd); }

// gidx[p]: where a wave's slot holds parameter p's gradient.  false if out of range or not one-to-one
inline bool grad_index(const Plan& pl, std::vector<int32_t>& gidx) {
  gidx.assign((size_t)pl.nparam, -1);
  for (int l = 0; l < pl.nl; l++) {
    const int in = pl.width[l], ou = pl.width[l + 1];
    for (int r = 0; r < ou; r++) {
      for (int c = 0; c < in; c++) gidx[pl.pw[l] + r * in + c] = slot_pos(pl.sw[l], l == 0 ? 1 : 4, r, c);
      gidx[pl.pb[l] + r] = pl.sb[l] + r;
    }
  }
  const int nti = 2 + pl.ntl;
  for (int i = 0; i < pl.nz; i++) {
    for (int j = 0; j < pl.nz; j++) gidx[pl.pA + i * pl.nz + j] = slot_pos(pl.sA, nti, z_pad(pl, i), z_pad(pl, j));
    for (int c = 0; c < pl.ud; c++) gidx[pl.pB + i * pl.ud + c] = slot_pos(pl.sA, nti, z_pad(pl, i), 16 * (1 + pl.ntl) + c);
  }
  if (pl.bil)
    for (int c = 0; c < pl.ud; c++)
      for (int i = 0; i < pl.nz; i++)
        for (int j = 0; j < pl.nz; j++)
          gidx[h_param(pl, c, i, j)] =
              slot_pos(pl.sH + c * (1 + pl.ntl) * (1 + pl.ntl) * 256, 1 + pl.ntl, z_pad(pl, i), z_pad(pl, j));
  std::vector<uint8_t> used((size_t)pl.slot_stride, 0);
  for (int p = 0; p < pl.nparam; p++) {
    if (gidx[p] < 0 || gidx[p] >= pl.slot_stride - 8 || used[gidx[p]]) return false;
    used[gidx[p]] = 1;
  }
  return true;
}

// the fragment blob of a parameter vector (zero padding)
inline void pack_blob(const Plan& pl, const std::vector<int32_t>& map, const double* params, std::vector<double>& blob) {
  blob.assign((size_t)pl.blob_total, 0.0);
  for (int c = 0; c < 2; c++)
    for (int p = 0; p < pl.nparam; p++) {
      const int32_t pos = map[(size_t)c * pl.nparam + p];
      if (pos >= 0) blob[pos] = params[p];
    }
}

// the argument checks of sim_koopman_loss_grad / sim_koopman_train_step (before any launch)
inline int check_step_args(const Plan& pl, int max_batch, int n, int N, int T, const void* rows, int ld, int x_off,
                           int u_off, bool has_idx, int t0, std::string& err) {
  if (!rows) return err = "null rows", SIM_E_ARG;
  if (n < 0) return err = "n must be >= 0", SIM_E_ARG;
  if (n > max_batch) return err = "n exceeds the trainer's max_batch", SIM_E_ARG;
  if (N < 1 || T < 0) return err = "N must be >= 1 and T >= 0", SIM_E_ARG;
  if (!has_idx && n > N) return err = "n exceeds N (traj_idx NULL reads trajectories 0..n-1)", SIM_E_ARG;
  if (t0 < 0 || (long long)t0 + pl.P > T) return err = "the window t0 .. t0 + pre_length runs past row T", SIM_E_ARG;
  if (ld < 1 || x_off < 0 || u_off < 0 || (long long)x_off + pl.xd > ld || (long long)u_off + pl.ud > ld)
    return err = "the x / u columns run past the row length ld", SIM_E_ARG;
  return SIM_OK;
}

}  // namespace ktrain
#endif  // KOOPMAN_TRAIN_PLAN_H
