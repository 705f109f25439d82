// tests/cpp/ingest_header.cc -- the two functions of include/flame_ros/image_io.h the ingest stage follows,
// toGray8 and undistort<uint8_t>, behind a file interface so that tests/test_ingest_ref.py can compare its NumPy restatement
// with them bit for bit.  Built with g++ -O2 -ffp-contract=off (every float operation rounded on its own, as on the GPU).
// Usage: ingest_header in.bin out.bin.  in.bin: int32 {mode, W, H, C}, float32 {fx, fy, cx, cy, k1, k2, p1, p2, k3}, then
// W x H x C bytes.  mode 0: toGray8 of the C-channel image (R, G, B[, A] order); mode 1: undistort<uint8_t> of the grey image
// (C = 1).  out.bin: W x H bytes.
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame_ros/image_io.h"

int main(int argc, char** argv) {
  if (argc < 3) return 10;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 11;
  int32_t hdr[4];
  float cam[9];
  if (std::fread(hdr, 4, 4, f) != 4 || std::fread(cam, 4, 9, f) != 9) return 11;
  const int mode = hdr[0], W = hdr[1], H = hdr[2], C = hdr[3];
  if (W < 1 || H < 1 || C < 1 || C > 4 || W > 8192 || H > 8192) return 11;
  std::vector<uint8_t> in(static_cast<size_t>(W) * H * C), out;
  if (std::fread(in.data(), 1, in.size(), f) != in.size()) return 11;
  std::fclose(f);
  namespace im = flame_ros::images;
  if (mode == 0) {
    im::Image img;
    img.width = W; img.height = H; img.channels = C; img.bit_depth = 8;
    img.u8 = in;
    if (!im::toGray8(img, &out)) return 12;
  } else if (mode == 1 && C == 1) {
    im::PlumbBob c;
    c.fx = cam[0]; c.fy = cam[1]; c.cx = cam[2]; c.cy = cam[3];
    c.k1 = cam[4]; c.k2 = cam[5]; c.p1 = cam[6]; c.p2 = cam[7]; c.k3 = cam[8];
    out.resize(in.size());
    im::undistort<uint8_t>(in.data(), W, H, 1, c, out.data());
  } else {
    return 13;
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 14;
  const bool ok = std::fwrite(out.data(), 1, out.size(), o) == out.size();
  std::fclose(o);
  return ok ? 0 : 14;
}
