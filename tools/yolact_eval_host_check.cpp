// Stand-alone host check of the YOLACT evaluation's arithmetic (csrc/yolact_eval_dev.h, the code
// tv_yolact_evaluate_match runs on the device: label and score of a softmax row, the score key and walk
// order, box and mask IoU) with the walk restated sequentially around it; no GPU and no Python. Meant for a
// sanitizer build of the host code, from tauv-vision_amd/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip \
//     ../tools/yolact_eval_host_check.cpp -o /tmp/yolact_eval_host_check && /tmp/yolact_eval_host_check cases.txt
// Input, whitespace separated, any number of images ("nan" is accepted):
//   C K N T, then T thresholds; K lines: C + 1 softmax values, box y x h w, det_area;
//   N lines: valid label y x h w truth_area; K lines of N intersections.
// Output per image: K lines "label score rank" followed by the 2 T truths the record took (-1: none), box
// kind first. Exit status 0 when every image was read whole; an incomplete image or a size outside the
// kernel's limits ends the run with status 1.
#include <cstdio>
#include <vector>

#include "../tauv-vision_amd/csrc/yolact_eval_dev.h"

int main(int argc, char** argv) {
  using namespace tv::yeval;
  std::FILE* in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!in) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 1;
  int C, K, N, T, images = 0;
  for (;;) {
    const int got = std::fscanf(in, "%d %d %d %d", &C, &K, &N, &T);
    if (got == EOF) break;
    if (got != 4 || C < 1 || C > 254 || K < 1 || K > 256 || N < 1 || N > 64 || T < 1 || T > 16)
      return std::fprintf(stderr, "image %d: header incomplete or outside the limits\n", images), 1;
    std::vector<float> thr(T), conf((size_t)K * (C + 1)), box((size_t)K * 4), tbox((size_t)N * 4);
    std::vector<int> det_area(K), valid(N), truth_area(N), inter((size_t)K * N);
    std::vector<long long> tlabel(N);
    bool ok = true;
    for (int j = 0; j < T; ++j) ok = ok && std::fscanf(in, "%f", &thr[j]) == 1;
    for (int i = 0; i < K && ok; ++i) {
      for (int c = 0; c <= C; ++c) ok = ok && std::fscanf(in, "%f", &conf[(size_t)i * (C + 1) + c]) == 1;
      for (int c = 0; c < 4; ++c) ok = ok && std::fscanf(in, "%f", &box[(size_t)i * 4 + c]) == 1;
      ok = ok && std::fscanf(in, "%d", &det_area[i]) == 1;
    }
    for (int t = 0; t < N && ok; ++t) {
      ok = ok && std::fscanf(in, "%d %lld", &valid[t], &tlabel[t]) == 2;
      for (int c = 0; c < 4; ++c) ok = ok && std::fscanf(in, "%f", &tbox[(size_t)t * 4 + c]) == 1;
      ok = ok && std::fscanf(in, "%d", &truth_area[t]) == 1;
    }
    for (size_t i = 0; i < inter.size() && ok; ++i) ok = ok && std::fscanf(in, "%d", &inter[i]) == 1;
    if (!ok) return std::fprintf(stderr, "image %d: incomplete\n", images), 1;

    std::vector<int> label(K), rank(K), order(K), took((size_t)K * 2 * T, -1);
    std::vector<float> score(K);
    std::vector<unsigned> key(K);
    for (int i = 0; i < K; ++i) {
      label_score(&conf[(size_t)i * (C + 1)], C, &label[i], &score[i]);
      key[i] = score_key(score[i]);
    }
    for (int i = 0; i < K; ++i) {
      rank[i] = 0;
      for (int j = 0; j < K; ++j) rank[i] += walks_before(key[j], j, key[i], i) ? 1 : 0;
      order[rank[i]] = i;
    }
    for (int kind = 0; kind < 2; ++kind)
      for (int j = 0; j < T; ++j) {
        std::vector<char> free_(N, 1);
        for (int r = 0; r < K; ++r) {
          const int i = order[r];
          int best = -1;
          double best_iou = 0.0;
          for (int t = 0; t < N; ++t) {
            if (!valid[t] || !free_[t] || tlabel[t] < 1 || tlabel[t] > C || tlabel[t] != (long long)label[i]) continue;
            const float* d = &box[(size_t)i * 4];
            const float* q = &tbox[(size_t)t * 4];
            const double iou = kind == 0 ? box_iou(d[0], d[1], d[2], d[3], q[0], q[1], q[2], q[3])
                                         : mask_iou(inter[(size_t)i * N + t], det_area[i], truth_area[t]);
            if (iou >= (double)thr[j] && (best < 0 || iou > best_iou)) { best = t; best_iou = iou; }
          }
          if (best >= 0) { free_[best] = 0; took[((size_t)i * 2 + kind) * T + j] = best; }
        }
      }
    for (int i = 0; i < K; ++i) {
      std::printf("%d %.9g %d", label[i], (double)score[i], rank[i]);
      for (int k = 0; k < 2 * T; ++k) std::printf(" %d", took[(size_t)i * 2 * T + k]);
      std::printf("\n");
    }
    ++images;
  }
  if (in != stdin) std::fclose(in);
  return 0;
}
