// initializer_driver.cc — csrc/two_view.h on the host behind a small main (tests/initializer_ref.py builds it with g++ and
// -ffp-contract=off; the sanitizer test builds it with -fsanitize=address,undefined; tools/bench_initializer.py times it).
//
//   initializer_driver IN OUT [REPEAT]
//
// IN:  int32 mode, n1, n2, n, n_hyp, kind; float sigma, K[9], model[9]; keys1 (n1 x 2 float), keys2, matches (n x 2 int32),
//      sets (n_hyp x 8 int32), subset ((n + 31) / 32 uint32)
// OUT: mode 0 (hypotheses):  model (2 x n_hyp x 9 float), score (2 x n_hyp float), n_inliers (2 x n_hyp int32), bits (2 x n_hyp x words)
//      mode 1 (reconstruct): decomposable (int32), R (8 x 9), t (8 x 3), n_good (8 int32), cos_sel (8 float), status (8 x n uint8),
//                            points (8 x n x 3 float), good_bits (8 x words); a fundamental matrix fills the first four of each
//      mode 2 (Initialize):  mode 0's output, then int32 best_h, best_f, kind, n_inliers of the kept hypothesis, motion, then mode 1's output
// REPEAT runs the computation that many times (for timing); the output is that of the last run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "two_view.h"

struct Problem {
    int32_t mode, n1, n2, n, n_hyp, kind;
    float sigma, K[9], model[9];
    std::vector<float> keys1, keys2;
    std::vector<int32_t> matches, sets;
    std::vector<uint32_t> subset;
    std::vector<float> m12;
    int words;
};

struct Hyp {
    std::vector<float> model, score;
    std::vector<int32_t> count;
    std::vector<uint32_t> bits;
};

struct Reco {
    int32_t decomposable;
    float R[72], t[24];
    int32_t n_good[8];
    float cos_sel[8];
    std::vector<uint8_t> status;
    std::vector<float> points;
    std::vector<uint32_t> good;
};

static void run_hyp(const Problem& P, Hyp& H) {
    const int nh = P.n_hyp, words = P.words;
    H.model.assign((size_t)2 * nh * 9, 0.f); H.score.assign((size_t)2 * nh, 0.f); H.count.assign((size_t)2 * nh, 0);
    H.bits.assign((size_t)2 * nh * words, 0u);
    const TvNorm n1 = tv_normalize(P.keys1.data(), P.n1), n2 = tv_normalize(P.keys2.data(), P.n2);
    const float inv_sigma2 = tv_inv_sigma2(P.sigma);
    const TvTeam T = {0, 1};
    TvWork W;
    for (int model = 0; model < 2; ++model)
        for (int h = 0; h < nh; ++h) {
            for (int j = 0; j < 8; ++j) tv_fill_pair(&W, model, j, &P.m12[4 * (size_t)P.sets[8 * (size_t)h + j]], n1, n2);
            float M[9], Mi[9];
            tv_model(T, &W, model, n1, n2, M, Mi);
            const size_t slot = (size_t)model * nh + h;
            float score = 0.f;
            int count = 0;
            for (int i = 0; i < P.n; ++i) {
                const TvTerms r = tv_check(model, M, Mi, &P.m12[4 * (size_t)i], inv_sigma2);
                if (r.ok1) score += r.t1;
                if (r.ok2) score += r.t2;
                if (r.ok1 && r.ok2) { H.bits[slot * words + (i >> 5)] |= 1u << (i & 31); ++count; }
            }
            memcpy(&H.model[9 * slot], M, sizeof(M));
            H.score[slot] = score; H.count[slot] = count;
        }
}

static void run_reco(const Problem& P, int kind, const float* model, const uint32_t* subset, Reco& R) {
    const int n = P.n, words = P.words;
    memset(R.R, 0, sizeof(R.R)); memset(R.t, 0, sizeof(R.t)); memset(R.n_good, 0, sizeof(R.n_good));
    for (int k = 0; k < 8; ++k) R.cos_sel[k] = 1.f;
    R.status.assign((size_t)8 * n, (uint8_t)TV_RT_NOT_INLIER); R.points.assign((size_t)8 * n * 3, 0.f); R.good.assign((size_t)8 * words, 0u);
    R.decomposable = 1;
    std::vector<uint32_t> keys;
    for (int mi = 0; mi < tv_motion_count(kind); ++mi) {
        TvMotion mo;
        const bool ok = tv_motion(kind, model, P.K, mi, &mo);
        memcpy(&R.R[9 * mi], mo.R, sizeof(mo.R)); memcpy(&R.t[3 * mi], mo.t, sizeof(mo.t));
        if (!ok) { R.decomposable = 0; continue; }
        TvCamera cam;
        tv_camera(P.K, mo, P.sigma, &cam);
        keys.clear();
        for (int i = 0; i < n; ++i) {
            if (!((subset[i >> 5] >> (i & 31)) & 1u)) continue;
            float X[3], c;
            bool good;
            const int st = tv_check_rt(cam, &P.m12[4 * (size_t)i], X, &c, &good);
            R.status[(size_t)mi * n + i] = (uint8_t)st;
            memcpy(&R.points[3 * ((size_t)mi * n + i)], X, sizeof(X));
            if (good) R.good[(size_t)mi * words + (i >> 5)] |= 1u << (i & 31);
            if (st == TV_RT_OK) {
                uint32_t b;
                memcpy(&b, &c, 4);
                keys.push_back(tv_cos_key(b));
            }
        }
        R.n_good[mi] = (int32_t)keys.size();
        if (!keys.empty()) {
            std::sort(keys.begin(), keys.end());
            const uint32_t b = tv_cos_unkey(keys[std::min<size_t>(50, keys.size() - 1)]);
            memcpy(&R.cos_sel[mi], &b, 4);
        }
    }
}

template <typename T>
static bool get(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

template <typename T>
static void put(FILE* f, const T* p, size_t count) {
    if (count) fwrite(p, sizeof(T), count, f);
}

static void put_hyp(FILE* f, const Hyp& H) {
    put(f, H.model.data(), H.model.size()); put(f, H.score.data(), H.score.size()); put(f, H.count.data(), H.count.size());
    put(f, H.bits.data(), H.bits.size());
}

static void put_reco(FILE* f, const Reco& R) {
    put(f, &R.decomposable, 1); put(f, R.R, 72); put(f, R.t, 24); put(f, R.n_good, 8); put(f, R.cos_sel, 8);
    put(f, R.status.data(), R.status.size()); put(f, R.points.data(), R.points.size()); put(f, R.good.data(), R.good.size());
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: initializer_driver IN OUT [REPEAT]\n"); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    Problem P;
    int32_t head[6];
    bool ok = fread(head, 4, 6, f) == 6;
    P.mode = head[0]; P.n1 = head[1]; P.n2 = head[2]; P.n = head[3]; P.n_hyp = head[4]; P.kind = head[5];
    ok = ok && P.n1 > 0 && P.n2 > 0 && P.n >= 8 && P.n_hyp >= 0;
    ok = ok && fread(&P.sigma, 4, 1, f) == 1 && fread(P.K, 4, 9, f) == 9 && fread(P.model, 4, 9, f) == 9;
    if (!ok) { fprintf(stderr, "bad header\n"); return 2; }
    P.words = (P.n + 31) / 32;
    ok = get(f, P.keys1, 2 * (size_t)P.n1) && get(f, P.keys2, 2 * (size_t)P.n2) && get(f, P.matches, 2 * (size_t)P.n) &&
         get(f, P.sets, 8 * (size_t)P.n_hyp) && get(f, P.subset, (size_t)P.words);
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    for (int i = 0; i < P.n; ++i)
        if (P.matches[2 * i] < 0 || P.matches[2 * i] >= P.n1 || P.matches[2 * i + 1] < 0 || P.matches[2 * i + 1] >= P.n2) { fprintf(stderr, "bad match\n"); return 2; }
    for (size_t k = 0; k < P.sets.size(); ++k)
        if (P.sets[k] < 0 || P.sets[k] >= P.n) { fprintf(stderr, "bad set\n"); return 2; }
    P.m12.resize(4 * (size_t)P.n);
    for (int i = 0; i < P.n; ++i) {
        const int a = P.matches[2 * i], b = P.matches[2 * i + 1];
        P.m12[4 * i] = P.keys1[2 * a]; P.m12[4 * i + 1] = P.keys1[2 * a + 1]; P.m12[4 * i + 2] = P.keys2[2 * b]; P.m12[4 * i + 3] = P.keys2[2 * b + 1];
    }
    Hyp H;
    Reco R;
    int32_t pick[5] = {-1, -1, 0, 0, -1};
    for (int rep = 0; rep < repeat; ++rep) {
        if (P.mode == 0 || P.mode == 2) run_hyp(P, H);
        if (P.mode == 1) run_reco(P, P.kind, P.model, P.subset.data(), R);
        if (P.mode == 2) {
            const int bh = tv_best_hypothesis(P.n_hyp, H.score.data()), bf = tv_best_hypothesis(P.n_hyp, H.score.data() + P.n_hyp);
            const float SH = bh >= 0 ? H.score[bh] : 0.f, SF = bf >= 0 ? H.score[P.n_hyp + bf] : 0.f;
            const int kind = tv_choose_h(SH, SF) ? TV_MODEL_H : TV_MODEL_F, b = kind == TV_MODEL_H ? bh : bf;
            const float zero[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const std::vector<uint32_t> none((size_t)P.words, 0u);
            const size_t slot = (size_t)kind * P.n_hyp + (b >= 0 ? b : 0);
            run_reco(P, kind, b >= 0 ? &H.model[9 * slot] : zero, b >= 0 ? &H.bits[slot * P.words] : none.data(), R);
            const int N = b >= 0 ? H.count[slot] : 0;
            float par[8];
            for (int k = 0; k < 8; ++k) par[k] = tv_parallax_deg(R.n_good[k], R.cos_sel[k]);
            int motion = -1;
            if (R.decomposable) motion = kind == TV_MODEL_H ? tv_pick_h(R.n_good, par, N, 1.0f, 50) : tv_pick_f(R.n_good, par, N, 1.0f, 50);
            pick[0] = bh; pick[1] = bf; pick[2] = kind; pick[3] = N; pick[4] = motion;
        }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    if (P.mode == 0 || P.mode == 2) put_hyp(o, H);
    if (P.mode == 2) put(o, pick, 5);
    if (P.mode == 1 || P.mode == 2) put_reco(o, R);
    fclose(o);
    return 0;
}
