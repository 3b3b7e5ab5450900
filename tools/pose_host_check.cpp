// Stand-alone host check of the pose numerics (csrc/pose_dev.h, the code tv_solve_poses runs on the
// device): solves cases read from a text file (argument) or from standard input, no GPU and no Python.
// Meant for a sanitizer build of the host code, from tauv-vision_amd/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip \
//     ../tools/pose_host_check.cpp -o /tmp/pose_host_check && /tmp/pose_host_check cases.txt
// Input, whitespace separated, any number of cases:
//   n fx fy cx cy min_points          then n lines   X Y Z u v
// (object point, pixel; "nan" is accepted). The object points and the camera are rounded to fp32 first, as
// the model table and the entry's arguments hold them; a pixel is taken as given (the kernel forms it in
// double from an fp32 record value and the frame size). Output: one line of the 16 pose columns per case
// (R row-major, t, valid, n, rms, LM iterations), "%.9g". Exit status 0 when every case was read whole (an
// invalid pose is a result, not an error); an incomplete case or n outside 0..32 ends the run with status 1.
#include <cstdio>
#include <cstdlib>

#include "../tauv-vision_amd/csrc/pose_dev.h"

int main(int argc, char** argv) {
  std::FILE* in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!in) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 1;
  static tv::pose::Work W;
  int n, min_points, cases = 0;
  double fx, fy, cx, cy;
  for (;;) {
    const int got = std::fscanf(in, "%d %lf %lf %lf %lf %d", &n, &fx, &fy, &cx, &cy, &min_points);
    if (got == EOF) break;
    if (got != 6) return std::fprintf(stderr, "case %d: header incomplete\n", cases), 1;
    if (n < 0 || n > tv::pose::kMaxPts) return std::fprintf(stderr, "case %d: n = %d outside 0..32\n", cases, n), 1;
    for (int k = 0; k < n; ++k) {
      double X[3], u, v;
      if (std::fscanf(in, "%lf %lf %lf %lf %lf", &X[0], &X[1], &X[2], &u, &v) != 5)
        return std::fprintf(stderr, "case %d: point %d incomplete\n", cases, k), 1;
      for (int i = 0; i < 3; ++i) W.X[k][i] = (double)(float)X[i];
      W.u[k] = u;
      W.v[k] = v;
    }
    const tv::pose::Result r = tv::pose::solve(W, n, (double)(float)fx, (double)(float)fy, (double)(float)cx,
                                               (double)(float)cy, min_points, tv::pose::Lanes{0, 1});
    float row[tv::pose::kCols];
    tv::pose::store_row(r, n, row);
    for (int i = 0; i < tv::pose::kCols; ++i) std::printf(i ? " %.9g" : "%.9g", (double)row[i]);
    std::printf("\n");
    ++cases;
  }
  if (in != stdin) std::fclose(in);
  return 0;
}
