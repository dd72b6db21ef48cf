// kfdb.hip — the keyframe database on the device (include/slamit.h, slamit_kfdb_*): what KeyFrameDatabase::DetectLoopCandidates and
// DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:84-206, :208-328) take from the inverted file and from
// L1Scoring::score (Thirdparty/DBoW2/src/ScoringObject.cpp:23-68).
//
// No inverted file: a slot is one row of word ids and one row of values (the keyframe's BowVector as slamit_voc_transform writes it),
// and a query is compared with every row.  One wavefront per (query, keyframe): each lane takes one of the keyframe's entries, 64
// coalesced per round, and binary-searches the query in LDS: n x 12 bytes, read once per workgroup of 16 keyframes, a sixteenth of
// what the rows cost.  (Searching a batch's queries through L2 instead took 2.1 times as long, profiles/r12_kfdb.json.)  The ballot of
// the hits gives the round's share of `common`, the first set bit of the first
// non-empty round the smallest shared word, and the terms of the hit lanes are added in lane order over the set bits only: the
// keyframe's entries ascend, so that is L1Scoring::score's order -- one term per shared word in ascending word id, from 0.0 -- and the
// double equals the reference's bit for bit.  No atomics, no LDS beyond the query, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "wave_ops.h"

struct slamit_kfdb {
    int device;
    int max_kf, max_words, n_live;
    int* words;              // [max_kf][max_words]
    double* values;          // [max_kf][max_words]
    int* n;                  // [max_kf]: the slot's entries, -1 = dead.  On the device, so add_dev never reads it back
    std::vector<unsigned char> live;
    std::vector<int64_t> seq;
    int64_t next_seq;        // never goes back: clear() and erase() leave it
    hipEvent_t wrote, read;  // after the last add_dev / query_batch_dev: what the next call of the other kind waits for
    bool wrote_pending, read_pending;
};

struct KfdbQuery {
    const int* qn; const int* qword; const double* qvalue; int cap;     // query q: qword + q * cap, qn[q] entries
    const int* kn; const int* kword; const double* kvalue; int max_kf, max_words;
    int* common; int* first_word; double* score;                         // [nq][max_kf]
};

#define KFDB_THREADS 1024
#define KFDB_WAVES (KFDB_THREADS / 64)

// first position of qw[0, n) that is not below w
__device__ __forceinline__ int kfdb_lower_bound(const int* qw, int n, int w) {
    int lo = 0, len = n;
    while (len > 0) {
        const int half = len >> 1;
        const bool right = qw[lo + half] < w;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo;
}

// LDS: values[cap] | words[cap] of the block's query
__global__ __launch_bounds__(KFDB_THREADS) void kfdb_query_kernel(KfdbQuery Q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kfdb_lds[];
    const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n = Q.qn[q];
    if (n < 0 || n > Q.cap) n = 0;                  // block-uniform: a count the transform did not write is an empty vector
    const int* gw = Q.qword + (size_t)q * Q.cap;
    const double* gv = Q.qvalue + (size_t)q * Q.cap;
    double* lv = reinterpret_cast<double*>(kfdb_lds);
    int* lw = reinterpret_cast<int*>(lv + Q.cap);
    for (int i = threadIdx.x; i < n; i += KFDB_THREADS) { lv[i] = gv[i]; lw[i] = gw[i]; }
    __syncthreads();
    for (int slot = blockIdx.x * KFDB_WAVES + wave; slot < Q.max_kf; slot += gridDim.x * KFDB_WAVES) {   // wave-uniform
        const int m = min(Q.kn[slot], Q.max_words);
        const size_t row = (size_t)slot * Q.max_words, out = (size_t)q * Q.max_kf + slot;
        int common = m < 0 ? -1 : 0, first = -1;
        double sum = 0.0;                           // ScoringObject.cpp:32
        for (int b = 0; b < m; b += 64) {
            const int e = b + lane;
            bool hit = false;
            int w = 0;
            double term = 0.0;
            if (e < m) {
                w = Q.kword[row + e];
                const int p = kfdb_lower_bound(lw, n, w);
                if (p < n && lw[p] == w) {
                    hit = true;
                    const double vi = lv[p], wi = Q.kvalue[row + e];
                    term = fabs(vi - wi) - fabs(vi) - fabs(wi);   // :41, left to right; no product in it, and -ffp-contract=off
                }
            }
            unsigned long long mask = __ballot(hit);
            if (mask == 0) continue;
            if (first < 0) first = __builtin_amdgcn_readlane(w, __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(mask)));   // entries ascend: the first hit is the smallest
            common += __popcll(mask);
            while (mask) {                          // shared words are a few percent of a vector: walk the set bits only
                sum += readlane_dyn_d(term, (int)__builtin_ctzll(mask));
                mask &= mask - 1;
            }
        }
        if (lane == 0) {
            Q.common[out] = common;
            Q.first_word[out] = first;
            Q.score[out] = common >= 1 ? -sum / 2.0 : 0.0;   // :65
        }
    }
}

// one frame's BowVector, as the transform wrote it, into a slot
__global__ __launch_bounds__(256) void kfdb_store_kernel(const int* d_n, const int* d_word, const double* d_value, int* words, double* values,
                                                         int* n_slot, int max_words) {
    int n = *d_n;
    if (n < 0 || n > max_words) n = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { words[i] = d_word[i]; values[i] = d_value[i]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_slot = n;
}

static size_t kfdb_query_lds(int cap) { return (size_t)cap * 12 + 8; }

// the dense pass of nq queries on stream st; the caller has made db->device current
static hipError_t kfdb_launch(const slamit_kfdb* db, KfdbQuery Q, int nq, hipStream_t st) {
    Q.kn = db->n; Q.kword = db->words; Q.kvalue = db->values; Q.max_kf = db->max_kf; Q.max_words = db->max_words;
    const int blocks = (db->max_kf + KFDB_WAVES - 1) / KFDB_WAVES;
    const size_t lds = kfdb_query_lds(Q.cap);       // <= 96 KiB: cap <= SLAMIT_VOC_MAX_FEATURES
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfdb_query_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kfdb_query_kernel, dim3(blocks < 1024 ? blocks : 1024, nq), dim3(KFDB_THREADS), lds, st, Q);
    return hipGetLastError();
}

// strictly ascending, non-negative word ids: what a std::map<WordId, WordValue> iterates
static bool kfdb_bow_ok(const int32_t* w, int n) {
    for (int i = 0; i < n; ++i)
        if (w[i] < 0 || (i > 0 && w[i] <= w[i - 1])) return false;
    return true;
}

static int kfdb_check_bow(const char* where, const int32_t* bow_word, const double* bow_value, int n) {
    if (n < 0 || (n > 0 && (!bow_word || !bow_value))) return slamit_fail(SLAMIT_ERR_ARG, (std::string(where) + ": bad vector").c_str());
    if (!kfdb_bow_ok(bow_word, n)) return slamit_fail(SLAMIT_ERR_ARG, (std::string(where) + ": word ids are not strictly ascending").c_str());
    return SLAMIT_OK;
}

// host writes to the rows wait for what add_dev / query_batch_dev have queued
static hipError_t kfdb_settle(slamit_kfdb* db) {
    hipError_t e = hipSuccess;
    if (db->wrote_pending) { e = hipEventSynchronize(db->wrote); db->wrote_pending = false; }
    if (e == hipSuccess && db->read_pending) { e = hipEventSynchronize(db->read); db->read_pending = false; }
    return e;
}

static int kfdb_free_slot(const slamit_kfdb* db) {
    for (int s = 0; s < db->max_kf; ++s)
        if (!db->live[s]) return s;
    return -1;
}

static int kfdb_full(const slamit_kfdb* db, const char* where) {
    return slamit_fail(SLAMIT_ERR_CAPACITY, (std::string(where) + ": the handle is full (max_kf = " + std::to_string(db->max_kf) + ")").c_str());
}

extern "C" int slamit_kfdb_create(int max_kf, int max_words, int device, slamit_kfdb** out) {
    if (!out) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_create: null argument");
    *out = nullptr;
    if (max_kf < 1 || max_words < 1) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_create: max_kf and max_words must be at least 1");
    if (max_words > SLAMIT_VOC_MAX_FEATURES) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_create: max_words > SLAMIT_VOC_MAX_FEATURES");
    SLAMIT_USE_DEVICE(device);
    slamit_kfdb* db = new slamit_kfdb();
    db->device = device; db->max_kf = max_kf; db->max_words = max_words; db->n_live = 0;
    db->words = nullptr; db->values = nullptr; db->n = nullptr; db->wrote = nullptr; db->read = nullptr;
    db->live.assign(max_kf, 0); db->seq.assign(max_kf, -1); db->next_seq = 0;
    db->wrote_pending = db->read_pending = false;
    const size_t cells = (size_t)max_kf * max_words;
    hipError_t e = hipMalloc((void**)&db->words, cells * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&db->values, cells * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&db->n, (size_t)max_kf * sizeof(int));
    if (e == hipSuccess) e = hipMemset(db->n, 0xFF, (size_t)max_kf * sizeof(int));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&db->wrote, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&db->read, hipEventDisableTiming);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (db->read) hipEventDestroy(db->read);
        if (db->wrote) hipEventDestroy(db->wrote);
        if (db->n) hipFree(db->n);
        if (db->values) hipFree(db->values);
        if (db->words) hipFree(db->words);
        delete db;
        return slamit_fail_hip(e, "slamit_kfdb_create");
    }
    *out = db;
    return SLAMIT_OK;
}

extern "C" void slamit_kfdb_destroy(slamit_kfdb* db) {
    if (!db) return;
    {
        SlamitDeviceGuard g(db->device);
        if (g.err == hipSuccess) {
            hipDeviceSynchronize();
            hipEventDestroy(db->read); hipEventDestroy(db->wrote);
            hipFree(db->n); hipFree(db->values); hipFree(db->words);
        }
    }
    delete db;
}

extern "C" int slamit_kfdb_clear(slamit_kfdb* db) {
    if (!db) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_clear: null handle");
    SLAMIT_USE_DEVICE(db->device);
    HIP_TRY_AT("slamit_kfdb_clear", kfdb_settle(db));
    HIP_TRY_AT("slamit_kfdb_clear", hipMemset(db->n, 0xFF, (size_t)db->max_kf * sizeof(int)));
    HIP_TRY_AT("slamit_kfdb_clear", hipDeviceSynchronize());
    db->live.assign(db->max_kf, 0); db->seq.assign(db->max_kf, -1); db->n_live = 0;
    return SLAMIT_OK;
}

extern "C" int slamit_kfdb_info(const slamit_kfdb* db, int32_t* max_kf, int32_t* max_words, int32_t* n_live) {
    if (!db) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_info: null handle");
    if (max_kf) *max_kf = db->max_kf;
    if (max_words) *max_words = db->max_words;
    if (n_live) *n_live = db->n_live;
    return SLAMIT_OK;
}

extern "C" int slamit_kfdb_add(slamit_kfdb* db, const int32_t* bow_word, const double* bow_value, int n, int32_t* slot) {
    const int rc = kfdb_check_bow("slamit_kfdb_add", bow_word, bow_value, n);   // before the handle: validation is host work
    if (rc != SLAMIT_OK) return rc;
    if (!db || !slot) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_add: null argument");
    if (n > db->max_words) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_kfdb_add: n > max_words");
    const int s = kfdb_free_slot(db);
    if (s < 0) return kfdb_full(db, "slamit_kfdb_add");
    SLAMIT_USE_DEVICE(db->device);
    HIP_TRY_AT("slamit_kfdb_add", kfdb_settle(db));
    const size_t row = (size_t)s * db->max_words;
    if (n > 0) {
        HIP_TRY_AT("slamit_kfdb_add", hipMemcpy(db->words + row, bow_word, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
        HIP_TRY_AT("slamit_kfdb_add", hipMemcpy(db->values + row, bow_value, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    }
    HIP_TRY_AT("slamit_kfdb_add", hipMemcpy(db->n + s, &n, sizeof(int), hipMemcpyHostToDevice));
    db->live[s] = 1; db->seq[s] = db->next_seq++; ++db->n_live;
    *slot = s;
    return SLAMIT_OK;
}

extern "C" int slamit_kfdb_add_dev(slamit_kfdb* db, const int32_t* d_bow_n, const int32_t* d_bow_word, const double* d_bow_value,
                                   void* stream, int32_t* slot) {
    if (!db || !slot || !d_bow_n || !d_bow_word || !d_bow_value) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_add_dev: null argument");
    const int s = kfdb_free_slot(db);
    if (s < 0) return kfdb_full(db, "slamit_kfdb_add_dev");
    SLAMIT_USE_DEVICE(db->device);
    hipStream_t st = (hipStream_t)stream;
    if (db->read_pending) HIP_TRY_AT("slamit_kfdb_add_dev", hipStreamWaitEvent(st, db->read, 0));
    if (db->wrote_pending) HIP_TRY_AT("slamit_kfdb_add_dev", hipStreamWaitEvent(st, db->wrote, 0));
    const size_t row = (size_t)s * db->max_words;
    const int blocks = (db->max_words + 255) / 256;
    hipLaunchKernelGGL(kfdb_store_kernel, dim3(blocks < 8 ? blocks : 8), dim3(256), 0, st, d_bow_n, d_bow_word, d_bow_value, db->words + row,
                       db->values + row, db->n + s, db->max_words);
    HIP_TRY_AT("slamit_kfdb_add_dev", hipGetLastError());
    HIP_TRY_AT("slamit_kfdb_add_dev", hipEventRecord(db->wrote, st));
    db->wrote_pending = true;
    db->live[s] = 1; db->seq[s] = db->next_seq++; ++db->n_live;
    *slot = s;
    return SLAMIT_OK;
}

extern "C" int slamit_kfdb_erase(slamit_kfdb* db, int slot) {
    if (!db) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_erase: null handle");
    if (slot < 0 || slot >= db->max_kf || !db->live[slot]) return SLAMIT_OK;   // KeyFrameDatabase.cc:56-75 on an absent keyframe
    SLAMIT_USE_DEVICE(db->device);
    HIP_TRY_AT("slamit_kfdb_erase", kfdb_settle(db));
    const int dead = -1;
    HIP_TRY_AT("slamit_kfdb_erase", hipMemcpy(db->n + slot, &dead, sizeof(int), hipMemcpyHostToDevice));
    db->live[slot] = 0; db->seq[slot] = -1; --db->n_live;
    return SLAMIT_OK;
}

extern "C" int slamit_kfdb_query(slamit_kfdb* db, const int32_t* bow_word, const double* bow_value, int n, int32_t* common,
                                 int32_t* first_word, int64_t* seq, double* score) {
    const int rc = kfdb_check_bow("slamit_kfdb_query", bow_word, bow_value, n);
    if (rc != SLAMIT_OK) return rc;
    if (!db || !common || !first_word || !score) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_query: null argument");
    if (n > SLAMIT_VOC_MAX_FEATURES) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_kfdb_query: n > SLAMIT_VOC_MAX_FEATURES");
    SLAMIT_USE_DEVICE(db->device);
    const size_t N = n, K = db->max_kf;
    StageLayout L;
    const StageSpan<double> qv = L.take<double>(N);
    const StageSpan<int> qw = L.take<int>(N), qn = L.take<int>(1);
    L.end_inputs();
    const StageSpan<double> os = L.take<double>(K);
    const StageSpan<int> oc = L.take<int>(K), of = L.take<int>(K);
    L.end_outputs();
    static thread_local SlamitScratch S;
    HIP_TRY_AT("slamit_kfdb_query: scratch", slamit_stage_reserve(S, db->device, L));
    if (n > 0) {
        memcpy(qv.at(S.host), bow_value, qv.bytes());
        memcpy(qw.at(S.host), bow_word, qw.bytes());
    }
    *qn.at(S.host) = n;
    if (db->wrote_pending) HIP_TRY_AT("slamit_kfdb_query", hipStreamWaitEvent(S.st, db->wrote, 0));
    HIP_TRY_AT("slamit_kfdb_query", slamit_stage_upload(S, L));
    KfdbQuery Q;
    Q.qn = qn.at(S.dev); Q.qword = qw.at(S.dev); Q.qvalue = qv.at(S.dev); Q.cap = n;
    Q.common = oc.at(S.dev); Q.first_word = of.at(S.dev); Q.score = os.at(S.dev);
    HIP_TRY_AT("slamit_kfdb_query", kfdb_launch(db, Q, 1, S.st));
    HIP_TRY_AT("slamit_kfdb_query", slamit_stage_download_and_wait(S, L));
    db->wrote_pending = false;                       // the stream waited for it and has finished
    memcpy(common, oc.at(S.host), oc.bytes());
    memcpy(first_word, of.at(S.host), of.bytes());
    memcpy(score, os.at(S.host), os.bytes());
    if (seq) memcpy(seq, db->seq.data(), sizeof(int64_t) * K);
    return SLAMIT_OK;
}

extern "C" int slamit_kfdb_query_batch_dev(slamit_kfdb* db, const int32_t* d_bow_n, const int32_t* d_bow_word, const double* d_bow_value,
                                           int cap, int nq, int32_t* d_common, int32_t* d_first_word, double* d_score, void* stream) {
    if (!db || cap < 0 || nq < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_query_batch_dev: bad argument");
    if (nq == 0) return SLAMIT_OK;
    if (!d_bow_n || !d_bow_word || !d_bow_value || !d_common || !d_first_word || !d_score)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_kfdb_query_batch_dev: null array");
    if (cap > SLAMIT_VOC_MAX_FEATURES) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_kfdb_query_batch_dev: cap > SLAMIT_VOC_MAX_FEATURES");
    if (nq > 65535) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_kfdb_query_batch_dev: more than 65535 queries in one call");
    SLAMIT_USE_DEVICE(db->device);
    hipStream_t st = (hipStream_t)stream;
    if (db->wrote_pending) HIP_TRY_AT("slamit_kfdb_query_batch_dev", hipStreamWaitEvent(st, db->wrote, 0));
    KfdbQuery Q;
    Q.qn = d_bow_n; Q.qword = d_bow_word; Q.qvalue = d_bow_value; Q.cap = cap;
    Q.common = d_common; Q.first_word = d_first_word; Q.score = d_score;
    HIP_TRY_AT("slamit_kfdb_query_batch_dev", kfdb_launch(db, Q, nq, st));
    HIP_TRY_AT("slamit_kfdb_query_batch_dev", hipEventRecord(db->read, st));
    db->read_pending = true;
    return SLAMIT_OK;
}
