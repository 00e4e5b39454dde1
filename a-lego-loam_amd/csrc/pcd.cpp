// pcd.cpp — alego_write_pcd: a cloud as PCD v0.7, binary (pcl::io::savePCDFileBinary's layout for PointXYZI without padding), the
// file format of saveMapCB (laserMapping.cpp:869-872).  Binary keeps every float bit-exact; PCL, Open3D and CloudCompare read it.
#include <cstdio>
#include <string>

#include "../../include/alego_mi355x.h"

extern "C" int alego_write_pcd(const char* path, const alego_point* pts, int32_t n) {
  if (!path || n < 0 || (n > 0 && !pts)) return ALEGO_ERR_ARG;
  FILE* f = std::fopen(path, "wb");
  if (!f) return ALEGO_ERR_ARG;
  const std::string hdr = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH " +
                          std::to_string(n) + "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " + std::to_string(n) + "\nDATA binary\n";
  bool ok = std::fwrite(hdr.data(), 1, hdr.size(), f) == hdr.size();
  if (ok && n > 0) ok = std::fwrite(pts, sizeof(alego_point), (size_t)n, f) == (size_t)n;
  ok = (std::fclose(f) == 0) && ok;
  return ok ? 0 : ALEGO_ERR_ARG;
}
