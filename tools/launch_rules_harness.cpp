// launch_rules_harness.cpp — prints what the launch rules of csrc/layout.hpp
// (general_variant, wide_rows, the dynamic LDS sizes) give for one small
// problem shape, as key=value words.  Host only: g++, no HIP.
// tests/test_launch_rules.py compares with hand-computed values.
#include <cstdio>
#include <cstring>

#include "../karpenter-provider-ibm-cloud_amd/csrc/encode.hpp"
#include "../karpenter-provider-ibm-cloud_amd/csrc/layout.hpp"

static gsd::DevProblem shape() {
  gsd::DevProblem d;
  std::memset(&d, 0, sizeof d);
  d.max_claims = 10;
  d.max_claims_wave = 7;
  d.n_thr = 5;
  d.nb_words = 3;
  d.NN = 4;
  d.TGZ = 2;
  d.ZS = 3;
  d.TGH = 1;
  d.ovh_slots = 16;
  return d;
}

int main() {
  gsd::DevProblem d = shape();
  std::printf("topo=%u block=%u sim=%u wave=%u wave_ch=%u", gsd::topo_lds_bytes(d), gsd::block_lds_bytes(d),
              gsd::sim_lds_bytes(d), gsd::wave_lds_bytes(d, false), gsd::wave_lds_bytes(d, true));
  d.sim_lds = 1;
  std::printf(" sim_queue=%u", gsd::sim_lds_bytes(d));
  std::printf(" sim_args=%u sim_args_queue=%u", gsd::sim_lds_bytes(880, 16, 10, false), gsd::sim_lds_bytes(880, 16, 10, true));
  d.n_lazy = 65;
  std::printf(" topo_lazy=%u", gsd::topo_lds_bytes(d));
  d.TGZ = d.TGH = 0;
  std::printf(" block_plain=%u", gsd::block_lds_bytes(d));

  // the variant rule, on the device record and on the encoder's
  gsd::DevProblem p = shape();
  gsh::Encoded e;
  std::printf(" none=%d%d", (int)gsd::general_variant(p), (int)gsd::general_variant(e));
  p.TG = e.TG = 1;
  std::printf(" tg=%d%d", (int)gsd::general_variant(p), (int)gsd::general_variant(e));
  p.TG = e.TG = 0;
  p.any_mv = 1;
  e.any_mv = true;
  std::printf(" mv=%d%d", (int)gsd::general_variant(p), (int)gsd::general_variant(e));
  p.any_mv = 0;
  e.any_mv = false;
  p.any_vol = 1;
  e.any_vol = true;
  std::printf(" vol=%d%d", (int)gsd::general_variant(p), (int)gsd::general_variant(e));
  e.TGZ = 2, e.ZS = 3, e.TGH = 1;
  std::printf(" topo_enc=%u", gsd::topo_lds_bytes(e));

  std::printf(" wide4=%d wide5=%d\n", (int)gsd::wide_rows(4), (int)gsd::wide_rows(5));
  return 0;
}
