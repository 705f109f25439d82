// tools/ingest_bench.cc -- host cost of what the ingest stage replaces: include/flame_ros/image_io.h toGray8 and
// undistort<uint8_t> on ONE thread, the way tools/flame_offline_lite.cc runs them per frame.  Built and run by
// tools/ingest_bench.py (g++ -O2).
// Usage: ingest_bench W H channels reps fx fy cx cy k1 k2 p1 p2 k3 -> one line: gray_us <median> undistort_us <median>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flame_ros/image_io.h"

int main(int argc, char** argv) {
  if (argc < 14) return 2;
  const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), C = std::atoi(argv[3]), reps = std::atoi(argv[4]);
  if (W < 1 || H < 1 || W > 8192 || H > 8192 || (C != 1 && C != 3 && C != 4) || reps < 1) return 2;
  namespace im = flame_ros::images;
  im::PlumbBob cam;
  float* dst[9] = {&cam.fx, &cam.fy, &cam.cx, &cam.cy, &cam.k1, &cam.k2, &cam.p1, &cam.p2, &cam.k3};
  for (int k = 0; k < 9; ++k) *dst[k] = static_cast<float>(std::atof(argv[5 + k]));
  im::Image raw;
  raw.width = W; raw.height = H; raw.channels = C; raw.bit_depth = 8;
  raw.u8.resize(raw.samples());
  uint32_t s = 12345u;
  for (size_t k = 0; k < raw.u8.size(); ++k) { s = s * 1664525u + 1013904223u; raw.u8[k] = static_cast<uint8_t>(s >> 24); }
  std::vector<uint8_t> gray, out(static_cast<size_t>(W) * H);
  std::vector<double> tg, tu;
  unsigned sink = 0;
  for (int r = 0; r < reps + 3; ++r) {
    raw.u8[static_cast<size_t>(r) % raw.u8.size()] ^= 1;  // (a new frame every time)
    const auto t0 = std::chrono::steady_clock::now();
    im::toGray8(raw, &gray);
    const auto t1 = std::chrono::steady_clock::now();
    im::undistort<uint8_t>(gray.data(), W, H, 1, cam, out.data());
    const auto t2 = std::chrono::steady_clock::now();
    sink += out[static_cast<size_t>(r * 7919) % out.size()] + gray[static_cast<size_t>(r * 104729) % gray.size()];
    if (r >= 3) {  // (warm-up: page faults of the first passes)
      tg.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
      tu.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
    }
  }
  std::sort(tg.begin(), tg.end());
  std::sort(tu.begin(), tu.end());
  std::printf("gray_us %.1f undistort_us %.1f sink %u\n", tg[tg.size() / 2], tu[tu.size() / 2], sink);
  return 0;
}
