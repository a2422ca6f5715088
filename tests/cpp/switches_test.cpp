// CPU test of rolo_amd/csrc/switches.hpp (the one table of switches the library reads from the environment): prints the table parsed from the environment it was started with,
// one "NAME value" line per switch; tests/test_switches.py compares the lines with what the hand-written parses this header replaced gave.
//   g++ -std=c++17 -I rolo_amd/csrc tests/cpp/switches_test.cpp -o switches_test && ROLO_LM_THREADS=768 ./switches_test
#include <cstdio>
#include "switches.hpp"

int main() {
  const rolo::Switches& s = rolo::switches();
  std::printf("ROLO_VOXEL_FUSE %d\nROLO_KNN_MOMENTS %d\nROLO_KNN_SUB %d\nROLO_POLAR_EXACT %d\n", s.voxel_fuse, s.knn_moments, s.knn_sub, s.polar_exact);
  std::printf("ROLO_LM_FUSED %d\nROLO_LM_THREADS %d\nROLO_LM_PPT %d\nROLO_LM_SPEC_LIN %d\nROLO_PASS_NRM %d\nROLO_PASS_XCD %d\nROLO_STAMP %d\n", s.lm_fused, s.lm_threads, s.lm_ppt, s.lm_spec_lin,
              s.pass_nrm, s.pass_xcd, s.stamp);
  std::printf("ROLO_LM_PERSIST_WGS %d\nROLO_LM_PERSIST_BUSY_THREADS %d\nROLO_LM_PERSIST_ADMIT_US %ld\nROLO_LM_PERSIST_TIMEOUT_MS %ld\n", s.lm_persist_wgs, s.lm_persist_busy_threads,
              s.lm_persist_admit_us, s.lm_persist_timeout_ms);
  std::printf("ROLO_LM_PERSIST_INTERLEAVE %d\nROLO_LM_PERSIST_MCACHE %d\nROLO_LM_PERSIST_BATCH %d\nROLO_CTRL_GENERIC %d\n", s.lm_persist_interleave, s.lm_persist_mcache, s.lm_persist_batch,
              s.ctrl_generic);
  std::printf("ROLO_CU_PARTITION %d\nROLO_ODOM_FRONT_PRIORITY %d\n", s.cu_partition, s.odom_front_priority);
  std::printf("ROLO_S2M_PACKETS %d\nROLO_S2M_STATS %s\n", s.s2m_packets, s.s2m_stats ? s.s2m_stats : "-");
  // the three that are read on every call
  std::printf("ROLO_PEER_TIMEOUT_MS %g\nROLO_PEER_MEM %s\nROLO_ODOM_EARLY_SOURCE %d/%d\n", rolo::peer_timeout_ms_now(), rolo::peer_mem_now() ? rolo::peer_mem_now() : "-",
              rolo::odom_early_source_now(false), rolo::odom_early_source_now(true));
  return 0;
}
