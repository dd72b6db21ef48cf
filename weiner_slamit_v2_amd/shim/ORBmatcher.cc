// ORBmatcher.cc — see ORBmatcher.h.  Distances and selection run in libslamit_hip.so; the
// acceptance thresholds and the rotation histogram are host logic as in the reference.
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

const int ORBmatcher::TH_HIGH = 100;     // ORBmatcher.cc:37
const int ORBmatcher::TH_LOW = 50;       // :38
const int ORBmatcher::HISTO_LENGTH = shim::RotationHistogram::LENGTH; // :39

ORBmatcher::ORBmatcher(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri), mbDeviceProjection(false) {}
ORBmatcher::ORBmatcher(float nnratio, bool checkOri, bool deviceProjection)
    : mfNNratio(nnratio), mbCheckOrientation(checkOri), mbDeviceProjection(deviceProjection) {}

namespace {
// descriptor tables may be row-padded cv::Mat views; the C-ABI wants 32-byte rows
const uint8_t* packed_rows(const cv::Mat& m, std::vector<uint8_t>& tmp) {
    if (m.rows == 0) return 0;
    if (m.isContinuous() && m.cols == SLAMIT_DESC_BYTES) return m.ptr<uint8_t>(0);
    tmp.resize((size_t)m.rows * SLAMIT_DESC_BYTES);
    for (int r = 0; r < m.rows; ++r) memcpy(&tmp[(size_t)r * SLAMIT_DESC_BYTES], m.ptr<uint8_t>(r), SLAMIT_DESC_BYTES);
    return tmp.data();
}
}  // namespace

int ORBmatcher::DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
    unsigned short d = 0;
    if (slamit_hamming_matrix(a.ptr<uint8_t>(0), 1, b.ptr<uint8_t>(0), 1, &d) != SLAMIT_OK) return 256;
    return d;
}

bool ORBmatcher::DistanceMatrix(const cv::Mat& query, const cv::Mat& train, std::vector<unsigned short>& dist) {
    std::vector<uint8_t> tq, tt;
    dist.assign((size_t)query.rows * train.rows, 0);
    return slamit_hamming_matrix(packed_rows(query, tq), query.rows, packed_rows(train, tt), train.rows, dist.data()) == SLAMIT_OK;
}

bool ORBmatcher::BestTwo(const cv::Mat& query, const cv::Mat& train, std::vector<int>& bestIdx,
                         std::vector<int>& bestDist, std::vector<int>& secondDist) {
    std::vector<uint8_t> tq, tt;
    bestIdx.assign(query.rows, -1); bestDist.assign(query.rows, 256); secondDist.assign(query.rows, 256);
    if (query.rows == 0) return true;
    return slamit_hamming_best2(packed_rows(query, tq), query.rows, packed_rows(train, tt), train.rows, bestIdx.data(),
                                bestDist.data(), secondDist.data()) == SLAMIT_OK;
}

int ORBmatcher::LastStatus() { return shim::status<ORBmatcher>(); }
void ORBmatcher::setStatus(int rc) { shim::status<ORBmatcher>() = rc; }

bool ORBmatcher::GuidedSearch(const std::vector<cv::KeyPoint>& keysUn, const cv::Mat& descriptors,
                              const std::vector<uint8_t>& kpTaken, float minX, float minY, float invW, float invH,
                              const GuidedQueries& q, int thDist, bool useRatio, float nnratio, std::vector<int>& matchKp,
                              float chi2Gate, const std::vector<float>* invLevelSigma2, int mode, std::vector<int>* acceptedKp,
                              const StereoGate* stereo) {
    const int n = (int)keysUn.size(), m = q.size();
    matchKp.assign(m, -1);
    setStatus(SLAMIT_OK);
    if (m == 0) return true;
    std::vector<float> xy(2 * (size_t)n);
    std::vector<int32_t> oct(n);
    for (int i = 0; i < n; ++i) { xy[2 * i] = keysUn[i].pt.x; xy[2 * i + 1] = keysUn[i].pt.y; oct[i] = keysUn[i].octave; }
    std::vector<uint8_t> td;
    slamit_frame_view fv;
    fv.n = n; fv.kp_xy = xy.data(); fv.kp_octave = oct.data(); fv.desc = n ? packed_rows(descriptors, td) : nullptr;
    fv.kp_taken = kpTaken.data(); fv.min_x = minX; fv.min_y = minY; fv.inv_w = invW; fv.inv_h = invH;
    slamit_search_queries sq;
    sq.m = m; sq.uvr = q.uvr.data(); sq.level_min = q.lmin.data(); sq.level_max = q.lmax.data(); sq.desc = q.desc.data();
    sq.valid = q.valid.data(); sq.takes = q.takes.data();
    slamit_search_rule rule;
    rule.th_dist = thDist; rule.use_ratio = useRatio ? 1 : 0; rule.nnratio = nnratio;
    rule.chi2_gate = chi2Gate;
    rule.mode = mode;
    for (int i = 0; i < 16; ++i) rule.inv_level_sigma2[i] = (invLevelSigma2 && i < (int)invLevelSigma2->size()) ? (*invLevelSigma2)[i] : 1.f;
    int nm = 0;
    if (acceptedKp) acceptedKp->assign(m, -1);
    if (stereo && stereo->erMode != SLAMIT_SEARCH_ER_NONE) {
        slamit_search_stereo st;
        st.er_mode = stereo->erMode; st.chi2_gate_stereo = stereo->chi2GateStereo;
        st.kp_ur = stereo->kpUr.data(); st.q_ur = q.ur.data(); st.q_ur_stride = 1;
        if ((int)stereo->kpUr.size() != n || (int)q.ur.size() != m) { setStatus(SLAMIT_ERR_ARG); return false; }
        setStatus(slamit_guided_search_stereo(0, &fv, &sq, &rule, &st, matchKp.data(), &nm, nullptr, acceptedKp ? acceptedKp->data() : nullptr, nullptr, nullptr));
        return LastStatus() == SLAMIT_OK;
    }
    setStatus(slamit_guided_search(0, &fv, &sq, &rule, matchKp.data(), &nm, nullptr, acceptedKp ? acceptedKp->data() : nullptr, nullptr, nullptr));
    return LastStatus() == SLAMIT_OK;
}

bool ORBmatcher::Project(std::vector<ProjectPoints>& batch) {
    setStatus(SLAMIT_OK);
    std::vector<slamit_project_problem> P(batch.size());
    std::vector<slamit_project_result> R(batch.size());
    for (size_t k = 0; k < batch.size(); ++k) {
        ProjectPoints& b = batch[k];
        const size_t n = (size_t)b.size();
        b.status.assign(n, 0); b.valid.assign(n, 0); b.proj.assign(2 * n, 0.f); b.uvr.assign(3 * n, 0.f);
        b.level.assign(n, 0); b.lmin.assign(n, 0); b.lmax.assign(n, 0);
        P[k].camera = b.cam; P[k].n = (int32_t)n;
        P[k].pos = b.pos.data(); P[k].normal = b.normal.data(); P[k].max_dist = b.maxd.data(); P[k].min_dist = b.mind.data();
        P[k].octave = b.octave.data(); P[k].skip = b.skip.data();
        R[k].status = b.status.data(); R[k].proj = b.proj.data(); R[k].level = b.level.data(); R[k].uvr = b.uvr.data();
        R[k].level_min = b.lmin.data(); R[k].level_max = b.lmax.data(); R[k].valid = b.valid.data(); R[k].n_valid = 0;
    }
    bool wantUr = false;
    for (size_t k = 0; k < batch.size(); ++k) wantUr = wantUr || batch[k].wantUr;
    if (wantUr) {   // one camera of the batch searches a stereo frame: every problem gets its ur (bf = 0 and unread for the others)
        std::vector<float> bf(batch.size());
        std::vector<float*> ur(batch.size());
        for (size_t k = 0; k < batch.size(); ++k) {
            batch[k].ur.assign((size_t)batch[k].size() + 1, 0.f);   // + 1: never a null pointer for an empty problem
            batch[k].wantUr = true;
            bf[k] = batch[k].bf; ur[k] = batch[k].ur.data();
        }
        const int rc = slamit_project_batch_stereo(0, (int)batch.size(), P.data(), R.data(), bf.data(), ur.data());
        if (rc != SLAMIT_OK) { shim::report<ORBmatcher>("slamit_project_batch_stereo", rc); return false; }
        return true;
    }
    const int rc = slamit_project_batch(0, (int)batch.size(), P.data(), R.data());
    if (rc != SLAMIT_OK) { shim::report<ORBmatcher>("slamit_project_batch", rc); return false; }
    return true;
}

bool ORBmatcher::BowSearch(const cv::Mat& desc1, const std::vector<uint8_t>& valid1, const cv::Mat& desc2, const std::vector<uint8_t>* valid2,
                           const BowGroups& g, int th, bool thInclusive, float nnratio, const EpipolarGate* gate, std::vector<int>& match12) {
    const int n1 = desc1.rows, n2 = desc2.rows;
    match12.assign(n1, -1);
    setStatus(SLAMIT_OK);
    if (n1 == 0 || n2 == 0 || g.size() == 0) return true;
    std::vector<uint8_t> t1, t2;
    slamit_bow_groups gg;
    gg.n_groups = g.size(); gg.q_ptr = g.q_ptr.data(); gg.q_idx = g.q_idx.data(); gg.c_ptr = g.c_ptr.data(); gg.c_idx = g.c_idx.data();
    slamit_bow_rule rule;
    memset(&rule, 0, sizeof(rule));
    rule.mode = gate ? 1 : 0; rule.th = th; rule.th_inclusive = thInclusive ? 1 : 0; rule.nnratio = nnratio;
    std::vector<float> xy1, xy2;
    std::vector<int32_t> oct2;
    if (gate) {
        memcpy(rule.F12, gate->F12, sizeof(rule.F12)); rule.ex = gate->ex; rule.ey = gate->ey;
        xy1.resize(2 * (size_t)n1); xy2.resize(2 * (size_t)n2); oct2.resize(n2);
        for (int i = 0; i < n1; ++i) { xy1[2 * i] = (*gate->keys1)[i].pt.x; xy1[2 * i + 1] = (*gate->keys1)[i].pt.y; }
        for (int i = 0; i < n2; ++i) { xy2[2 * i] = (*gate->keys2)[i].pt.x; xy2[2 * i + 1] = (*gate->keys2)[i].pt.y; oct2[i] = (*gate->keys2)[i].octave; }
        rule.kp1_xy = xy1.data(); rule.kp2_xy = xy2.data(); rule.kp2_octave = oct2.data();
        for (int i = 0; i < 16; ++i) {
            rule.scale_factor[i] = i < (int)gate->scaleFactors->size() ? (*gate->scaleFactors)[i] : 1.f;
            rule.level_sigma2[i] = i < (int)gate->levelSigma2->size() ? (*gate->levelSigma2)[i] : 1.f;
        }
    }
    int nm = 0;
    if (gate && gate->uRight1 && gate->uRight2) {
        if ((int)gate->uRight1->size() < n1 || (int)gate->uRight2->size() < n2) { shim::refuse<ORBmatcher>("SearchForTriangulation: mvuRight is shorter than N"); return false; }
        slamit_bow_stereo st;
        st.ur1 = gate->uRight1->data(); st.ur2 = gate->uRight2->data(); st.only_stereo = gate->onlyStereo ? 1 : 0;
        setStatus(slamit_bow_search_stereo(0, packed_rows(desc1, t1), n1, valid1.empty() ? nullptr : valid1.data(), packed_rows(desc2, t2), n2,
                                           valid2 ? valid2->data() : nullptr, &gg, &rule, &st, match12.data(), nullptr, &nm));
        return LastStatus() == SLAMIT_OK;
    }
    setStatus(slamit_bow_search(0, packed_rows(desc1, t1), n1, valid1.empty() ? nullptr : valid1.data(), packed_rows(desc2, t2), n2,
                                valid2 ? valid2->data() : nullptr, &gg, &rule, match12.data(), nullptr, &nm));
    return LastStatus() == SLAMIT_OK;
}

int ORBmatcher::SearchBruteForce(const std::vector<cv::KeyPoint>& keys1, const cv::Mat& desc1,
                                 const std::vector<cv::KeyPoint>& keys2, const cv::Mat& desc2,
                                 std::vector<int>& vnMatches12, int th) {
    if (th < 0) th = TH_LOW;
    std::vector<int> idx, best, second;
    vnMatches12.assign(desc1.rows, -1);
    if (!BestTwo(desc1, desc2, idx, best, second)) return 0;
    shim::RotationHistogram rotHist;
    int nmatches = 0;
    for (int i = 0; i < desc1.rows; ++i) {
        if (best[i] <= th && (float)best[i] < mfNNratio * (float)second[i]) {
            vnMatches12[i] = idx[i];
            ++nmatches;
            if (mbCheckOrientation && i < (int)keys1.size() && idx[i] < (int)keys2.size()) rotHist.add(keys1[i].angle, keys2[idx[i]].angle, i);
        }
    }
    if (mbCheckOrientation)
        rotHist.reject([&](int i) {
            if (vnMatches12[i] >= 0) { vnMatches12[i] = -1; --nmatches; }
        });
    return nmatches;
}

// part of the reference's surface; the searches go through shim::RotationHistogram
void ORBmatcher::ComputeThreeMaxima(std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3) {
    shim::RotationHistogram::ThreeMaxima(histo, L, ind1, ind2, ind3);
}

}  // namespace ORB_SLAM2
