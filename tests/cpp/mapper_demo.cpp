// C++ host-side check of rolo::MapOptimization (include/rolo_nodes_hip.hpp): a sequence of CloudInfoStamp feature clouds goes through laserCloudInfoHandler in a
// C++-only process (no Python / torch).
// Input: scans.bin = int32 n_scans, then per scan float64 stamp, int32 n_corner, int32 n_surf, n_corner x 4 float32, n_surf x 4 float32. Prints one line per scan:
// processed, transformTobeMapped[6], incremental6[6], the scan-to-submap stats, the sizes, the key frame.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rolo_nodes_hip.hpp"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: mapper_demo scans.bin [surf_leaf] [keyframe_density]\n"); return 1; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  rolo::MapperParams P;
  if (argc > 2) P.mappingSurfLeafSize = (float)std::atof(argv[2]);
  if (argc > 3) P.surroundingKeyframeDensity = (float)std::atof(argv[3]);
  int32_t ns = 0;
  if (std::fread(&ns, 4, 1, f) != 1) return 3;
  try {
    rolo::MapOptimization mapping(0, P);
    for (int k = 0; k < ns; k++) {
      double stamp = 0; int32_t nc = 0, nsf = 0;
      if (std::fread(&stamp, 8, 1, f) != 1 || std::fread(&nc, 4, 1, f) != 1 || std::fread(&nsf, 4, 1, f) != 1) return 3;
      std::vector<float> corner((size_t)nc * 4), surf((size_t)nsf * 4);
      if (std::fread(corner.data(), 16, nc, f) != (size_t)nc || std::fread(surf.data(), 16, nsf, f) != (size_t)nsf) return 3;
      const bool processed = mapping.laserCloudInfoHandler(stamp, corner, surf);
      const rolo_mapper_result& r = mapping.result;
      std::printf("%d", processed ? 1 : 0);
      for (float v : mapping.transformTobeMapped) std::printf(" %.9g", v);
      for (float v : r.incremental6) std::printf(" %.9g", v);
      std::printf(" %d %d %d %d %d %d %d %d %d %d\n", r.s2m_ran, r.s2m.skipped, r.s2m.iterations, r.s2m.converged, r.s2m.n_selected, r.n_corner_ds, r.n_surf_ds, r.m_corner,
                  r.m_surf, r.keyframe);
    }
    std::vector<float> pose6; std::vector<double> time;
    std::printf("keyposes %d\n", mapping.cloudKeyPoses6D(pose6, time));
    // error behaviour: misuse surfaces as rolo::Error with the ROLO_E* code
    const double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, bad[6] = {1, 1, 1, 1, 1, -1};
    try { mapping.queueLoop(0, 1, T, bad); std::printf("no-throw\n"); } catch (const rolo::Error& e) { std::printf("error %d\n", e.code); }
  } catch (const rolo::Error& e) {
    std::fprintf(stderr, "rolo::Error %d: %s\n", e.code, e.what());
    return 4;
  }
  std::fclose(f);
  return 0;
}
