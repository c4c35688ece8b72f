// koopman_layout.h — the host-side layout every Koopman unit packs its MFMA fragments by, said once:
// the shape checks of a sim_koopman_desc, the encoder's fragment layout, the padded k order and the
// fragment fill loop.  Plain C++ (no HIP), so tools/koopman_train_selftest.cpp runs it under the host
// sanitizers without a GPU.  Users: sim_koopman_create (koopman_mpc.hip), sim_koopman_set_model
// (koopman_predict.hip), sim_koopman_set_box (koopman_box.hip) and koopman_train_plan.h.
//
// A fragment is 64 lanes of one v_mfma_f64_16x16x4_f64 A operand: lane l holds
// M[16 T + (l & 15)][4 s + (l >> 4)] of output tile T and k-step s; a matrix is [ntile][ks][64].
// The lifted state z = [x | features] meets the kernels padded to whole operands:
//   rows   tile 0 = the x rows (x_dim of 16), tile 1 + q = features 16 q .. 16 q + 15;
//   k      [x (8) | features (16 ntl) | u (8)], the order the encoder leaves its B operands in.
#ifndef KOOPMAN_LAYOUT_H
#define KOOPMAN_LAYOUT_H

#include <cstddef>
#include <string>

#include "../../include/koopman_mpc.h"

constexpr size_t KOOPMAN_LDS_BYTES = 160 * 1024;  // the LDS of a CU: every kernel's dynamic-LDS limit

namespace klayout {

// the shape checks of a controller description: SIM_OK, or SIM_E_MODEL with its message in err
inline int check_desc(const sim_koopman_desc& d, std::string& err) {
  const int xd = d.x_dim, nl = d.nlayer;
  if (xd < 1 || xd > SIM_KMAXX) return err = "x_dim must be in 1..8", SIM_E_MODEL;
  if (d.u_dim < 1 || d.u_dim > SIM_KMAXU) return err = "u_dim must be in 1..8", SIM_E_MODEL;
  if (nl < 2 || nl > SIM_KMAXLAYER) return err = "nlayer must be in 2..6", SIM_E_MODEL;
  if (d.horizon < 1 || d.horizon > SIM_KMAXH) return err = "horizon must be in 1..32", SIM_E_MODEL;
  if (d.width[0] != xd) return err = "width[0] must equal x_dim", SIM_E_MODEL;
  for (int l = 1; l <= nl; l++)
    if (d.width[l] < 1 || d.width[l] > SIM_KMAXW) return err = "encoder widths must be in 1..64", SIM_E_MODEL;
  return SIM_OK;
}

// the encoder's part of a fragment blob (offsets in doubles), of a description check_desc accepted.
// Static kernel shapes: layer 0 = 4 tiles x 2 k-steps (x padded to 8), hidden = 4 x 16, last = ntl x 16
struct Encoder {
  int xd, ud, nl, outw, nz, ntl;  // outw: the last layer's width; nz = xd + outw; ntl: its 16-row tiles
  int ntile[SIM_KMAXLAYER], ks[SIM_KMAXLAYER], frag[SIM_KMAXLAYER];  // W_l: [ntile][ks][64] at frag
  int bias;                                                          // [nl][SIM_KMAXW]
  int total;                                                         // doubles of the above
};
inline Encoder encoder(const sim_koopman_desc& d) {
  Encoder e{};
  e.xd = d.x_dim, e.ud = d.u_dim, e.nl = d.nlayer, e.outw = d.width[e.nl], e.nz = e.xd + e.outw;
  int off = 0;
  for (int l = 0; l < e.nl; l++) {
    e.ntile[l] = l == e.nl - 1 ? (d.width[l + 1] + 15) / 16 : 4;
    e.ks[l] = l == 0 ? 2 : 16;
    e.frag[l] = off;
    off += e.ntile[l] * e.ks[l] * 64;
  }
  e.ntl = e.ntile[e.nl - 1];
  e.bias = off;
  e.total = off + e.nl * SIM_KMAXW;
  return e;
}

// k-steps of the padded k order: z alone, and with the inputs behind it
inline int ks_z(const Encoder& e) { return 2 + 4 * e.ntl; }
inline int ks_zu(const Encoder& e) { return 2 + 4 * e.ntl + 2; }

// lifted-state index of (tile, row in tile) / of padded k index kk; input index of kk; -1 = padding
inline int z_of_row(const Encoder& e, int tile, int r) {
  if (tile == 0) return r < e.xd ? r : -1;
  const int f = 16 * (tile - 1) + r;
  return (tile <= e.ntl && f < e.outw) ? e.xd + f : -1;
}
inline int z_of_k(const Encoder& e, int kk) {
  if (kk < 0) return -1;
  if (kk < 8) return kk < e.xd ? kk : -1;
  kk -= 8;
  return (kk < 16 * e.ntl && kk < e.outw) ? e.xd + kk : -1;
}
inline int u_of_k(const Encoder& e, int kk) {
  kk -= 8 + 16 * e.ntl;
  return (kk >= 0 && kk < e.ud) ? kk : -1;
}
// column of a matrix whose columns are [.. | z (nz, from zcol) | u (ud)] that padded k index kk reads
inline int zu_col(const Encoder& e, int kk, int zcol) {
  const int j = z_of_k(e, kk), c = u_of_k(e, kk);
  return j >= 0 ? zcol + j : (c >= 0 ? zcol + e.nz + c : -1);
}

// the fragment loop: f(pos, row, k) for every element of a [ntile][ks][64] fragment matrix, pos its
// offset in doubles, (row, k) = (16 T + (lane & 15), 4 s + (lane >> 4)) the matrix element it holds
template <class F>
inline void each_frag(int ntile, int ks, F&& f) {
  for (int T = 0; T < ntile; T++)
    for (int s = 0; s < ks; s++)
      for (int lane = 0; lane < 64; lane++) f((T * ks + s) * 64 + lane, 16 * T + (lane & 15), 4 * s + (lane >> 4));
}
// dst[pos] = f(row, k)
template <class F>
inline void fill_frag(double* dst, int ntile, int ks, F&& f) {
  each_frag(ntile, ks, [&](int pos, int row, int k) { dst[pos] = f(row, k); });
}

}  // namespace klayout
#endif  // KOOPMAN_LAYOUT_H
