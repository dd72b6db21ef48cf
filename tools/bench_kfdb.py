"""Times the keyframe database's dense query (slamit_kfdb_query_batch_dev) and sets it against a single-core host walk of the reference's
form: an inverted file of std::list plus one std::map merge per keyframe that shares a word.

    python tools/bench_kfdb.py [--reps 30] [--warmup 10] [--out profiles/r12_kfdb.json]

Cases: 2,000 and 8,000 keyframes x 1,000 words each, one query and 64 queries per call.  Word ids are drawn without repetition from a
pool of 20,000, so a pair shares 1000 x 1000 / 20000 = 50 words on average (the run records the range it saw; 20-100 is the aim).
Device events around `reps` back-to-back calls on one stream after `warmup` calls.  The bytes are the algorithmic ones, live slots x n x
12 B per query (a word id and a value per entry of every keyframe; the query's own 12 KB and the 20 B of output per slot are not
counted).  The comparator is written below, compiled with g++ -O3 on the same host and run on one core; its counts and score bits must
equal the device's, and the run says whether they do.  Recorded, not gated."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL, WORDS = 20000, 1000

COMPARATOR = r'''
// kfdb_cpu <dir> <n_kf> <n_words> <n_queries>: words.i32 / values.f64 [n_kf][n_words], qwords.i32 / qvalues.f64 [n_queries][n_words]
// -> common.i32, score.f64 [n_queries][n_kf] and, on stdout, the mean microseconds per query (walk + scores, one core).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <string>
#include <vector>
template <class T> static std::vector<T> slurp(const std::string& p, size_t n) {
    std::vector<T> v(n);
    FILE* f = fopen(p.c_str(), "rb");
    if (!f || fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "cannot read %s\n", p.c_str()); exit(2); }
    fclose(f);
    return v;
}
template <class T> static void dump(const std::string& p, const std::vector<T>& v) {
    FILE* f = fopen(p.c_str(), "wb");
    fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}
typedef std::map<unsigned, double> Bow;
int main(int argc, char** argv) {
    const std::string d = argv[1];
    const size_t K = atol(argv[2]), N = atol(argv[3]), Q = atol(argv[4]);
    const std::vector<int> w = slurp<int>(d + "/words.i32", K * N), qw = slurp<int>(d + "/qwords.i32", Q * N);
    const std::vector<double> x = slurp<double>(d + "/values.f64", K * N), qx = slurp<double>(d + "/qvalues.f64", Q * N);
    std::vector<Bow> kf(K), qs(Q);
    unsigned top = 0;
    for (size_t k = 0; k < K; ++k) for (size_t i = 0; i < N; ++i) { kf[k][w[k * N + i]] = x[k * N + i]; if ((unsigned)w[k * N + i] > top) top = w[k * N + i]; }
    for (size_t q = 0; q < Q; ++q) for (size_t i = 0; i < N; ++i) { qs[q][qw[q * N + i]] = qx[q * N + i]; if ((unsigned)qw[q * N + i] > top) top = qw[q * N + i]; }
    std::vector<std::list<int> > inverted(top + 1);
    for (size_t k = 0; k < K; ++k) for (Bow::const_iterator it = kf[k].begin(); it != kf[k].end(); ++it) inverted[it->first].push_back((int)k);
    std::vector<int> common(Q * K, 0), sharing;
    std::vector<double> score(Q * K, 0.0);
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t q = 0; q < Q; ++q) {
        int* c = &common[q * K];
        sharing.clear();
        for (Bow::const_iterator it = qs[q].begin(); it != qs[q].end(); ++it) {
            const std::list<int>& l = inverted[it->first];
            for (std::list<int>::const_iterator k = l.begin(); k != l.end(); ++k) if (c[*k]++ == 0) sharing.push_back(*k);
        }
        for (size_t s = 0; s < sharing.size(); ++s) {
            const Bow& b = kf[sharing[s]];
            Bow::const_iterator i = qs[q].begin(), j = b.begin();
            double sum = 0.0;
            while (i != qs[q].end() && j != b.end()) {
                if (i->first == j->first) { sum += fabs(i->second - j->second) - fabs(i->second) - fabs(j->second); ++i; ++j; }
                else if (i->first < j->first) i = qs[q].lower_bound(j->first);
                else j = b.lower_bound(i->first);
            }
            score[q * K + sharing[s]] = -sum / 2.0;
        }
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / Q;
    dump(d + "/common.i32", common);
    dump(d + "/score.f64", score);
    printf("%.3f\n", us);
    return 0;
}
'''


def vectors(rs, count):
    w = np.stack([np.sort(rs.permutation(POOL)[:WORDS]) for _ in range(count)]).astype(np.int32)
    v = rs.uniform(0.05, 9.0, (count, WORDS)) * rs.randint(1, 4, (count, WORDS))
    return w, np.ascontiguousarray(v / v.sum(1, keepdims=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_kfdb.json"))
    a = ap.parse_args()
    import torch

    from weiner_slamit_v2_amd import api

    if api.device_count() < 1:
        raise SystemExit("bench_kfdb: no HIP device (there is no CPU path to time)")
    tmp = tempfile.mkdtemp(prefix="kfdb_bench_")
    open(os.path.join(tmp, "kfdb_cpu.cc"), "w").write(COMPARATOR)
    exe = os.path.join(tmp, "kfdb_cpu")
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-ffp-contract=off", os.path.join(tmp, "kfdb_cpu.cc"), "-o", exe])
    res = {"workload": "slamit_kfdb_query_batch_dev: keyframes x %d words, word ids drawn without repetition from a pool of %d" % (WORDS, POOL),
           "timing": "device events around reps back-to-back calls on one stream, after warmup calls of the same shape",
           "bytes": "algorithmic: live slots x n x 12 B per query", "reps": a.reps, "warmup": a.warmup,
           "comparator": "single core, g++ -O3: std::list inverted file walk + std::map merge per sharing keyframe", "cases": []}
    rs = np.random.RandomState(12)
    qw, qv = vectors(rs, 64)
    for n_kf in (2000, 8000):
        kw, kv = vectors(rs, n_kf)
        db = api.KeyFrameDatabase(n_kf, WORDS)
        for k in range(n_kf):
            db.add(kw[k], kv[k])
        for name, arr in (("words.i32", kw), ("values.f64", kv), ("qwords.i32", qw), ("qvalues.f64", qv)):
            arr.tofile(os.path.join(tmp, name))
        cpu_us = float(subprocess.check_output([exe, tmp, str(n_kf), str(WORDS), "64"]).decode())
        c_common = np.fromfile(os.path.join(tmp, "common.i32"), np.int32).reshape(64, n_kf)
        c_score = np.fromfile(os.path.join(tmp, "score.f64"), np.float64).reshape(64, n_kf)
        for nq in (1, 64):
            t = {"bow_n": torch.full((nq,), WORDS, dtype=torch.int32, device="cuda"), "bow_word": torch.from_numpy(qw[:nq]).cuda(),
                 "bow_value": torch.from_numpy(qv[:nq]).cuda(), "common": torch.zeros((nq, n_kf), dtype=torch.int32, device="cuda"),
                 "first_word": torch.zeros((nq, n_kf), dtype=torch.int32, device="cuda"), "score": torch.zeros((nq, n_kf), dtype=torch.float64, device="cuda")}
            s = torch.cuda.Stream()
            for _ in range(a.warmup):
                db.query_batch_dev(t, stream=s.cuda_stream)
            s.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                for _ in range(a.reps):
                    db.query_batch_dev(t, stream=s.cuda_stream)
                e1.record()
            s.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            t0 = time.perf_counter()
            for _ in range(a.reps):
                host = db.query(qw[0], qv[0])
            host_ms = (time.perf_counter() - t0) / a.reps * 1e3
            common, score = t["common"].cpu().numpy(), t["score"].cpu().numpy()
            m = c_common[:nq] >= 1
            same = np.array_equal(common, c_common[:nq]) and np.array_equal(score[m].view(np.uint64), c_score[:nq][m].view(np.uint64))
            same = same and np.array_equal(host[0], c_common[0]) and np.array_equal(host[3].view(np.uint64), c_score[0].view(np.uint64))
            nbytes = n_kf * WORDS * 12 * nq
            res["cases"].append({"keyframes": n_kf, "words_per_keyframe": WORDS, "queries": nq, "ms_per_call": ms, "us_per_query": 1e3 * ms / nq,
                                 "algorithmic_bytes": nbytes, "achieved_TBs": nbytes / (ms * 1e-3) / 1e12,
                                 "ms_host_form_one_query_wall": host_ms, "cpu_us_per_query": cpu_us, "speedup_over_cpu": cpu_us / (1e3 * ms / nq),
                                 "shared_words_min_mean_max": [int(c_common[:nq].min()), float(c_common[:nq].mean()), int(c_common[:nq].max())],
                                 "equals_cpu_counts_and_score_bits": bool(same)})
        db.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
