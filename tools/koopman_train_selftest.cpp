// koopman_train_selftest.cpp — the Koopman trainer's host-side code (csrc/koopman_train_plan.h: the
// plan of the DKUC trainer and of the bilinear DBKN one, the fragment index map, the slot gather index,
// blob packing, the nmse workspace sizes, the per-step argument checks) and the layout every Koopman unit
// packs by (csrc/koopman_layout.h: the description's checks, the encoder layout, the padded row and k
// maps, the fragment loop) as a stand-alone program for the host sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/koopman_train_selftest.cpp -o /tmp/koopman_train_selftest && /tmp/koopman_train_selftest
//
// Prints "selftest ok" and exits 0; any mismatch aborts with a message.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "../lerobot-mujoco-sim2real_amd/csrc/koopman_train_plan.h"

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

static sim_koopman_desc desc_of(std::vector<int> w, int ud) {
  sim_koopman_desc d{};
  d.x_dim = w[0], d.u_dim = ud, d.nlayer = (int)w.size() - 1, d.horizon = 10, d.u_clip = 0.5;
  for (size_t i = 0; i < w.size(); i++) d.width[i] = w[i];
  return d;
}
static sim_koopman_train_opts opts_of(int P, int npos) {
  sim_koopman_train_opts o{};
  o.struct_size = sizeof(o), o.abi_version = SIM_ABI_VERSION;
  o.pre_length = P, o.npos = npos, o.gamma = 0.8, o.beta1 = 0.9, o.beta2 = 0.999, o.eps = 1e-8;
  return o;
}

static void check_shape(std::vector<int> w, int ud, int P) {
  using namespace ktrain;
  const sim_koopman_desc d = desc_of(w, ud);
  const sim_koopman_train_opts o = opts_of(P, 1);
  Plan pl;
  std::string err;
  REQUIRE(make_plan(d, o, pl, err) == SIM_OK);
  std::vector<int32_t> map, gidx;
  REQUIRE(index_map(pl, map));
  REQUIRE(grad_index(pl, gidx));
  REQUIRE((int)map.size() == 2 * pl.nparam && (int)gidx.size() == pl.nparam);
  std::vector<double> p(pl.nparam), blob;
  std::iota(p.begin(), p.end(), 1.0);  // parameter i holds i + 1: a blob value names its parameter
  pack_blob(pl, map, p.data(), blob);
  REQUIRE((int)blob.size() == pl.blob_total);
  // the encoder fragments as sim_koopman_create packs them, from the layout alone
  const int nl = pl.nl;
  for (int l = 0; l < nl; l++) {
    const int in = w[l], ou = w[l + 1];
    for (int T = 0; T < pl.ntile[l]; T++)
      for (int s = 0; s < pl.ks[l]; s++)
        for (int lane = 0; lane < 64; lane++) {
          const int row = 16 * T + (lane & 15), col = 4 * s + (lane >> 4);
          const double want = (row < ou && col < in) ? p[pl.pw[l] + row * in + col] : 0.0;
          REQUIRE(blob[pl.frag[l] + (T * pl.ks[l] + s) * 64 + lane] == want);
          if (l >= 1 && s < pl.kst[l] && T < 4) {  // W_l': row = an input, k = an output
            const int r2 = 16 * T + (lane & 15), k2 = 4 * s + (lane >> 4);
            const double wt = (r2 < in && k2 < ou) ? p[pl.pw[l] + k2 * in + r2] : 0.0;
            REQUIRE(blob[pl.wt[l] + (T * pl.kst[l] + s) * 64 + lane] == wt);
          }
        }
    for (int r = 0; r < SIM_KMAXW; r++) REQUIRE(blob[pl.bias + l * SIM_KMAXW + r] == (r < ou ? p[pl.pb[l] + r] : 0.0));
  }
  // [A | B] and A': tile 0 = the x rows, tile 1 + q = features 16 q ..; k order [x (8) | features | u (8)]
  const int xd = w[0], outw = w[nl], nz = xd + outw, ntl = pl.ntl;
  auto zrow = [&](int tile, int r) { return tile == 0 ? (r < xd ? r : -1) : (16 * (tile - 1) + r < outw ? xd + 16 * (tile - 1) + r : -1); };
  auto zk = [&](int kk) { return kk < 8 ? (kk < xd ? kk : -1) : (kk - 8 < 16 * ntl && kk - 8 < outw ? xd + kk - 8 : -1); };
  for (int tile = 0; tile <= ntl; tile++)
    for (int lane = 0; lane < 64; lane++) {
      for (int s = 0; s < pl.abks; s++) {
        const int i = zrow(tile, lane & 15), kk = 4 * s + (lane >> 4), j = zk(kk), c = kk - 8 - 16 * ntl;
        double want = 0.0;
        if (i >= 0 && kk < 8 + 16 * ntl && j >= 0) want = p[pl.pA + i * nz + j];
        if (i >= 0 && c >= 0 && c < ud) want = p[pl.pB + i * ud + c];
        REQUIRE(blob[pl.ab + (tile * pl.abks + s) * 64 + lane] == want);
      }
      for (int s = 0; s < pl.atks; s++) {
        const int j = zrow(tile, lane & 15), i = zk(4 * s + (lane >> 4));
        REQUIRE(blob[pl.at + (tile * pl.atks + s) * 64 + lane] == ((i >= 0 && j >= 0) ? p[pl.pA + i * nz + j] : 0.0));
      }
    }
  // sizes the kernels rely on
  REQUIRE(pl.enc_total % 2 == 0 && pl.lds_bytes <= LDS_BYTES);
  REQUIRE(pl.abks % 4 == 0 && pl.atks % 2 == 0);
  REQUIRE(pl.scr_stride == P * 2 * (1 + ntl) * 256 + (MAXL - 1) * 1024);
  for (int q = 0; q < pl.nparam; q++) REQUIRE(gidx[q] >= 0 && gidx[q] + 8 < pl.slot_stride + 1);
  // the nmse workspace: every wave's [P][8] sums inside the stats buffer; the table [P][4] and the six
  // losses behind the step count, inside its buffer and clear of the count; the table kernel's LDS row
  for (int max_batch : {1, 16, 17, 130, 4096}) {
    const int max_slot = (max_batch + 15) / 16;
    REQUIRE(stat_doubles(pl, max_slot) == (size_t)max_slot * P * 8);
    REQUIRE(((size_t)(max_slot - 1) * P + (P - 1)) * 8 + 7 < stat_doubles(pl, max_slot));
  }
  REQUIRE(tab_doubles(pl) == (size_t)4 * P + 8 && pl.P <= MAXP);  // (the table kernel's LDS: [MAXP][8])
  REQUIRE(STEP_DOUBLES * sizeof(double) >= sizeof(int));
  REQUIRE(step_bytes(pl) == (STEP_DOUBLES + tab_doubles(pl)) * sizeof(double));
  REQUIRE((STEP_DOUBLES + (size_t)4 * (P - 1) + 3) * sizeof(double) < step_bytes(pl));  // the last coefficient
  REQUIRE((STEP_DOUBLES + (size_t)4 * P + 5) * sizeof(double) < step_bytes(pl));        // the last loss
  // the per-step argument checks
  float rows = 0;
  const int T = P + 3;
  REQUIRE(check_step_args(pl, 32, 16, 20, T, &rows, 13, 5, 0, false, 0, err) == SIM_OK);
  REQUIRE(check_step_args(pl, 32, 16, 20, T, &rows, 13, 5, 0, false, T - P, err) == SIM_OK);
  REQUIRE(check_step_args(pl, 32, 0, 20, T, &rows, 13, 5, 0, false, 0, err) == SIM_OK);
  REQUIRE(check_step_args(pl, 32, 16, 20, T, nullptr, 13, 5, 0, false, 0, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 33, 40, T, &rows, 13, 5, 0, false, 0, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, -1, 20, T, &rows, 13, 5, 0, false, 0, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 16, 20, T, &rows, 13, 5, 0, false, -1, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 16, 20, T, &rows, 13, 5, 0, false, T - P + 1, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 16, 20, T, &rows, 13, 5, 0, false, 2147483647, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 16, 20, T, &rows, 13, 13 - xd + 1, 0, false, 0, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 16, 20, T, &rows, 13, 5, 13 - ud + 1, false, 0, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 16, 20, T, &rows, 2147483647, 2147483647 - 2, 0, false, 0, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 16, 8, T, &rows, 13, 5, 0, false, 0, err) == SIM_E_ARG);
  REQUIRE(check_step_args(pl, 32, 16, 8, T, &rows, 13, 5, 0, true, 0, err) == SIM_OK);
  REQUIRE(check_step_args(pl, 32, 16, 0, T, &rows, 13, 5, 0, true, 0, err) == SIM_E_ARG);
}

// the bilinear plan (DBKN): the linear plan's numbers unmoved, the H block of the parameter vector, the
// H_c / H_c' fragments against the packing rule restated, dH's slot, the maps one-to-one and in range
static void check_bilinear(std::vector<int> w, int ud, int P, int u_z) {
  using namespace ktrain;
  const sim_koopman_desc d = desc_of(w, ud);
  const sim_koopman_train_opts o = opts_of(P, 1);
  Plan lin, pl;
  std::string err;
  REQUIRE(make_plan(d, o, lin, err) == SIM_OK);
  REQUIRE(make_plan(d, o, pl, err, true, u_z) == SIM_OK);
  REQUIRE(!lin.bil && lin.hf == -1 && lin.ht == -1 && lin.pH == -1 && lin.sH == -1);
  const int nl = pl.nl, xd = w[0], outw = w[nl], nz = xd + outw, ntl = pl.ntl, nzt = 1 + ntl, atks = pl.atks;
  // the linear part is where the linear plan has it; the new blocks follow it
  REQUIRE(pl.bil == 1 && pl.uz == u_z && pl.ab == lin.ab && pl.at == lin.at && pl.pA == lin.pA && pl.pB == lin.pB);
  REQUIRE(pl.sA == lin.sA && pl.scr_stride == lin.scr_stride && pl.lds_bytes == lin.lds_bytes && pl.enc_total == lin.enc_total);
  for (int l = 0; l < nl; l++) REQUIRE(pl.pw[l] == lin.pw[l] && pl.sw[l] == lin.sw[l] && pl.frag[l] == lin.frag[l]);
  REQUIRE(pl.pH == lin.nparam && pl.nparam == lin.nparam + nz * nz * ud);
  REQUIRE(pl.hf == lin.blob_total && pl.hf == pl.at + nzt * atks * 64);  // (the kernel derives hf, ht, sH so)
  REQUIRE(pl.ht == pl.hf + ud * nzt * atks * 64 && pl.blob_total == pl.ht + ud * nzt * atks * 64);
  REQUIRE(pl.sH == pl.sA + nzt * (nzt + 1) * 256 && pl.sH == lin.slot_stride - 8);
  REQUIRE(pl.slot_stride == pl.sH + ud * nzt * nzt * 256 + 8);
  std::vector<int32_t> map, gidx, lmap, lgidx;
  REQUIRE(index_map(pl, map) && grad_index(pl, gidx));
  REQUIRE(index_map(lin, lmap) && grad_index(lin, lgidx));
  REQUIRE((int)map.size() == 2 * pl.nparam && (int)gidx.size() == pl.nparam);
  for (int p = 0; p < lin.nparam; p++)
    REQUIRE(map[p] == lmap[p] && map[pl.nparam + p] == lmap[lin.nparam + p] && gidx[p] == lgidx[p]);
  // every H parameter: exactly two copies, one in hf and one in ht; its gradient inside dH's region
  std::vector<char> seen(pl.slot_stride, 0);
  for (int p = pl.pH; p < pl.nparam; p++) {
    const int a = std::min(map[p], map[pl.nparam + p]), b = std::max(map[p], map[pl.nparam + p]);
    REQUIRE(a >= pl.hf && a < pl.ht && b >= pl.ht && b < pl.blob_total);
    REQUIRE(gidx[p] >= pl.sH && gidx[p] < pl.slot_stride - 8 && !seen[gidx[p]]);
    seen[gidx[p]] = 1;
  }
  std::vector<double> p(pl.nparam), blob;
  std::iota(p.begin(), p.end(), 1.0);
  pack_blob(pl, map, p.data(), blob);
  REQUIRE((int)blob.size() == pl.blob_total);
  auto zrow = [&](int tile, int r) { return tile == 0 ? (r < xd ? r : -1) : (16 * (tile - 1) + r < outw ? xd + 16 * (tile - 1) + r : -1); };
  auto zk = [&](int kk) { return kk < 8 ? (kk < xd ? kk : -1) : (kk - 8 < 16 * ntl && kk - 8 < outw ? xd + kk - 8 : -1); };
  // H_c[i][j], the factor of u_c z_j in row i, from net.H.weight (nz x nz ud row-major) in the u_z order
  auto Hc = [&](int c, int i, int j) { return p[pl.pH + i * nz * ud + (u_z ? c * nz + j : j * ud + c)]; };
  for (int c = 0; c < ud; c++)
    for (int tile = 0; tile < nzt; tile++)
      for (int s = 0; s < atks; s++)
        for (int lane = 0; lane < 64; lane++) {
          const int r = zrow(tile, lane & 15), k = zk(4 * s + (lane >> 4));
          const int o2 = ((c * nzt + tile) * atks + s) * 64 + lane;
          REQUIRE(blob[pl.hf + o2] == ((r >= 0 && k >= 0) ? Hc(c, r, k) : 0.0));
          REQUIRE(blob[pl.ht + o2] == ((r >= 0 && k >= 0) ? Hc(c, k, r) : 0.0));
        }
  // dH_c[i][j] in the slot: tile (row tile of i, column tile of j) of [c][nzt][nzt], C/D layout
  auto pad = [&](int z) { return z < xd ? z : 16 + (z - xd); };
  for (int c = 0; c < ud; c++)
    for (int i = 0; i < nz; i++)
      for (int j = 0; j < nz; j++) {
        const int ri = pad(i), cj = pad(j);
        const int want = pl.sH + (((c * nzt + ri / 16) * nzt + cj / 16) * 4 + (ri % 16) / 4) * 64 + (ri % 4) * 16 + cj % 16;
        REQUIRE(gidx[pl.pH + i * nz * ud + (u_z ? c * nz + j : j * ud + c)] == want);
      }
  // the linear blob is a prefix of the bilinear one
  std::vector<double> lblob;
  pack_blob(lin, lmap, p.data(), lblob);
  for (int q = 0; q < lin.blob_total; q++) REQUIRE(blob[q] == lblob[q]);
  REQUIRE(make_plan(d, o, pl, err, true, 2) == SIM_E_ARG && make_plan(d, o, pl, err, true, -1) == SIM_E_ARG);
  REQUIRE(make_plan(d, o, pl, err, false, 2) == SIM_OK && !pl.bil);  // (u_z is the bilinear plan's alone)
}

// koopman_layout.h, which every Koopman unit packs by: the padded row and k maps one-to-one onto the
// unpadded indices, the fragment loop against its element-wise definition, the encoder layout against
// the rule restated (and the trainer's plan, where it takes the shape)
static void check_layout(std::vector<int> w, int ud) {
  using namespace klayout;
  const sim_koopman_desc d = desc_of(w, ud);
  std::string err;
  REQUIRE(check_desc(d, err) == SIM_OK && err.empty());
  const Encoder e = encoder(d);
  const int nl = (int)w.size() - 1, xd = w[0], outw = w[nl], nz = xd + outw;
  REQUIRE(e.xd == xd && e.ud == ud && e.nl == nl && e.outw == outw && e.nz == nz && e.ntl == (outw + 15) / 16);
  int off = 0;
  for (int l = 0; l < nl; l++) {
    REQUIRE(e.ntile[l] == (l == nl - 1 ? (w[l + 1] + 15) / 16 : 4) && e.ks[l] == (l == 0 ? 2 : 16) && e.frag[l] == off);
    off += e.ntile[l] * e.ks[l] * 64;
  }
  REQUIRE(e.bias == off && e.total == off + nl * SIM_KMAXW && e.total % 2 == 0);
  REQUIRE(ks_z(e) == 2 + 4 * e.ntl && ks_zu(e) == ks_z(e) + 2);
  if (nl <= ktrain::MAXL) {
    ktrain::Plan pl;
    REQUIRE(ktrain::make_plan(d, opts_of(5, 1), pl, err) == SIM_OK);
    for (int l = 0; l < nl; l++) REQUIRE(pl.ntile[l] == e.ntile[l] && pl.ks[l] == e.ks[l] && pl.frag[l] == e.frag[l]);
    REQUIRE(pl.bias == e.bias && pl.enc_total == e.total && pl.ntl == e.ntl && pl.abks == ks_zu(e) && pl.atks == ks_z(e));
  }
  // rows: every lifted index once over tiles 0 .. ntl, in order; -1 on the padding and past the tiles
  std::vector<int> seen(nz, 0);
  for (int tile = 0; tile <= e.ntl + 1; tile++)
    for (int r = 0; r < 16; r++) {
      const int z = z_of_row(e, tile, r);
      const int want = tile == 0 ? (r < xd ? r : -1) : (tile <= e.ntl && 16 * (tile - 1) + r < outw ? xd + 16 * (tile - 1) + r : -1);
      REQUIRE(z == want && z < nz);
      if (z >= 0) seen[z]++;
    }
  for (int z = 0; z < nz; z++) REQUIRE(seen[z] == 1);
  // k: [x (8) | features (16 ntl) | u (8)]; every lifted index and every input once, never both
  std::vector<int> zs(nz, 0), us(ud, 0);
  for (int kk = -4; kk < 4 * ks_zu(e) + 8; kk++) {
    const int z = z_of_k(e, kk), u = u_of_k(e, kk), f = kk - 8, c = kk - 8 - 16 * e.ntl;
    REQUIRE(z == (kk >= 0 && kk < 8 ? (kk < xd ? kk : -1) : (f >= 0 && f < 16 * e.ntl && f < outw ? xd + f : -1)));
    REQUIRE(u == (c >= 0 && c < ud ? c : -1) && !(z >= 0 && u >= 0) && z < nz && u < ud);
    REQUIRE(zu_col(e, kk, 100) == (z >= 0 ? 100 + z : (u >= 0 ? 100 + nz + u : -1)));
    if (z >= 0) zs[z]++;
    if (u >= 0) us[u]++;
  }
  for (int z = 0; z < nz; z++) REQUIRE(zs[z] == 1);
  for (int u = 0; u < ud; u++) REQUIRE(us[u] == 1);
  // the fragment loop: lane l of fragment (T, s) holds element (16 T + (l & 15), 4 s + (l >> 4))
  for (int l = 0; l < nl; l++) {
    const int nt = e.ntile[l], ks = e.ks[l];
    std::vector<double> blob((size_t)nt * ks * 64, -1.0);
    fill_frag(blob.data(), nt, ks, [](int row, int k) { return 1000.0 * row + k; });
    for (int T = 0; T < nt; T++)
      for (int s = 0; s < ks; s++)
        for (int lane = 0; lane < 64; lane++)
          REQUIRE(blob[(T * ks + s) * 64 + lane] == 1000.0 * (16 * T + (lane & 15)) + 4 * s + (lane >> 4));
    std::vector<int> hit(blob.size(), 0);
    each_frag(nt, ks, [&](int pos, int row, int k) {
      REQUIRE(pos >= 0 && pos < (int)hit.size() && blob[pos] == 1000.0 * row + k);
      hit[pos]++;
    });
    for (int h : hit) REQUIRE(h == 1);
  }
}

static void check_desc_refusals() {
  using namespace klayout;
  const sim_koopman_desc good = desc_of({8, 64, 64, 24}, 5);
  std::string err;
  auto refused = [&](sim_koopman_desc d, const char* msg) {
    err.clear();
    REQUIRE(check_desc(d, err) == SIM_E_MODEL && err == msg);
  };
  sim_koopman_desc d = good;
  d.x_dim = 0, refused(d, "x_dim must be in 1..8");
  d.x_dim = SIM_KMAXX + 1, refused(d, "x_dim must be in 1..8");
  d = good, d.u_dim = 0, refused(d, "u_dim must be in 1..8");
  d.u_dim = SIM_KMAXU + 1, refused(d, "u_dim must be in 1..8");
  d = good, d.nlayer = 1, refused(d, "nlayer must be in 2..6");
  d.nlayer = SIM_KMAXLAYER + 1, refused(d, "nlayer must be in 2..6");
  d = good, d.horizon = 0, refused(d, "horizon must be in 1..32");
  d.horizon = SIM_KMAXH + 1, refused(d, "horizon must be in 1..32");
  d = good, d.width[0] = 7, refused(d, "width[0] must equal x_dim");
  d = good, d.width[2] = 0, refused(d, "encoder widths must be in 1..64");
  d = good, d.width[3] = SIM_KMAXW + 1, refused(d, "encoder widths must be in 1..64");
  // the same refusals reach the trainer's plan with their messages
  ktrain::Plan pl;
  d = good, d.u_dim = 9;
  REQUIRE(ktrain::make_plan(d, opts_of(5, 3), pl, err) == SIM_E_MODEL && err == "u_dim must be in 1..8");
  // the reference's encoder: the figures the kernels were written against
  const Encoder e = encoder(desc_of({8, 64, 64, 64, 64, 24}, 5));
  const int frag[5] = {0, 512, 4608, 8704, 12800};
  for (int l = 0; l < 5; l++) REQUIRE(e.frag[l] == frag[l]);
  REQUIRE(e.ntl == 2 && e.bias == 14848 && e.total == 15168 && e.nz == 32);
  REQUIRE(KOOPMAN_LDS_BYTES == 163840 && ktrain::LDS_BYTES == KOOPMAN_LDS_BYTES);
}

int main() {
  using namespace ktrain;
  // koopman_layout.h at the widths of the shape table's rows ref, nz45, odd, tiny, deep and nz3
  check_layout({8, 64, 64, 64, 64, 24}, 5);
  check_layout({8, 64, 37}, 5);
  check_layout({7, 33, 17, 22}, 3);
  check_layout({3, 6, 10}, 1);
  check_layout({5, 64, 64, 64, 64, 64, 9}, 4);
  check_layout({2, 1, 1}, 2);
  check_desc_refusals();
  for (int u_z = 0; u_z < 2; u_z++) {
    check_bilinear({8, 64, 64, 64, 64, 24}, 5, 5, u_z);  // the reference's shape
    check_bilinear({8, 64, 64, 40}, 5, 1, u_z);
    check_bilinear({8, 64, 64}, 8, 5, u_z);              // four feature tiles, the most inputs
    check_bilinear({3, 17, 5}, 1, 64, u_z);
    check_bilinear({8, 33, 64, 1, 16}, 3, 2, u_z);
  }
  check_shape({8, 64, 64, 64, 64, 24}, 5, 5);  // the reference's encoder
  check_shape({8, 64, 64, 40}, 5, 1);          // three last-layer tiles
  check_shape({8, 64, 64}, 5, 5);              // four
  check_shape({3, 17, 5}, 1, 64);              // odd widths, one tile, the longest window
  check_shape({8, 33, 64, 1, 16}, 8, 2);
  // refusals
  Plan pl;
  std::string err;
  sim_koopman_desc d = desc_of({8, 64, 64, 64, 64, 64, 24}, 5);
  sim_koopman_train_opts o = opts_of(5, 3);
  REQUIRE(make_plan(d, o, pl, err) == SIM_E_MODEL);  // nlayer 6
  d = desc_of({8, 64, 65}, 5);
  REQUIRE(make_plan(d, o, pl, err) == SIM_E_MODEL);
  d = desc_of({8, 64, 24}, 5);
  d.horizon = 0;
  REQUIRE(make_plan(d, o, pl, err) == SIM_E_MODEL);
  d.horizon = 10;
  for (int bad = 0; bad < 5; bad++) {
    o = opts_of(5, 3);
    if (bad == 0) o.pre_length = 0;
    if (bad == 1) o.pre_length = MAXP + 1;
    if (bad == 2) o.npos = 8;
    if (bad == 3) o.gamma = 0.0;
    if (bad == 4) o.beta2 = 1.0;
    REQUIRE(make_plan(d, o, pl, err) == SIM_E_ARG && !err.empty());
  }
  std::puts("selftest ok");
  return 0;
}
