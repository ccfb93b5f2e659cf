// Stages::relocalize composed from the fine-grained stages (the GPU-less harness under oracle/ compiles this file; no HIP here): detection on
// the whole image, description, the map's descriptor medoids, a host brute-force k = 2 match with the semantics of alva_reloc_match, and
// the pose solve in the order of the tracking step (track_default.cpp: P3P-LMedS, its outliers removed, robust PnP).
#include "se3.hpp"
#include "stages.hpp"
#include <climits>
#include <cmath>
#include <cstring>

namespace alva_slam {

int Stages::relocalize(const RelocJob &job, RelocResult &out) {
    out = RelocResult();
    if (image_width_ <= 0 || image_height_ <= 0 || job.cell <= 0) return -1;
    const int cells_w = (image_width_ + job.cell - 1) / job.cell, cells_h = (image_height_ + job.cell - 1) / job.cell;
    const int cap = cells_w * cells_h + 8;
    std::vector<float> pts((size_t) cap * 2);
    int n = 0;
    int rc = detect(job.cell, 0, nullptr, cap, pts.data(), &n);
    if (rc) return rc;
    n = n > cap ? cap : n;
    out.n_detect = n;
    if (n <= 0 || job.n_map <= 0) return 0;
    std::vector<uint8_t> desc((size_t) n * 32), valid((size_t) n);
    std::vector<float> unpx((size_t) n * 2);
    std::vector<double> bv((size_t) n * 3);
    rc = describe_and_compute(n, pts.data(), desc.data(), valid.data(), unpx.data(), bv.data());
    if (rc) return rc;
    const int m = job.n_map;
    std::vector<uint8_t> mdesc((size_t) m * 32), mvalid((size_t) m);
    std::vector<int> info((size_t) m * 3);
    rc = medoid_export(m, job.map_slot, mdesc.data(), mvalid.data(), info.data());
    if (rc) return rc;
    // k = 2 under (distance, id), ratio test, one-to-one by (distance, query index)
    std::vector<int> best_row((size_t) n, -1), best_d((size_t) n, 0);
    std::vector<long long> claim((size_t) m, LLONG_MAX);
    for (int q = 0; q < n; q++) {
        if (!valid[(size_t) q]) continue;
        int bd = 257, bid = INT_MAX, br = -1, bs = 257;
        const uint8_t *a = &desc[(size_t) q * 32];
        for (int r = 0; r < m; r++) {
            if (!mvalid[(size_t) r] || info[3 * (size_t) r] <= 0 || job.map_id[r] < 0) continue;
            const uint8_t *b = &mdesc[(size_t) r * 32];
            int d = 0;
            for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned) (a[k] ^ b[k]));
            const int id = job.map_id[r];
            if (d < bd || (d == bd && id < bid)) {
                bs = bd;
                bd = d; bid = id; br = r;
            } else if (d < bs) {
                bs = d;
            }
        }
        if (br >= 0 && bd <= job.max_dist && (float) bd < job.ratio * (float) bs) {
            best_row[(size_t) q] = br;
            best_d[(size_t) q] = bd;
            const long long key = ((long long) bd << 32) | q;
            if (key < claim[(size_t) br]) claim[(size_t) br] = key;
        }
    }
    std::vector<int> mq, mr;
    for (int q = 0; q < n; q++) {
        const int r = best_row[(size_t) q];
        if (r >= 0 && claim[(size_t) r] == (((long long) best_d[(size_t) q] << 32) | q)) {
            mq.push_back(q);
            mr.push_back(r);
        }
    }
    const int k = (int) mq.size();
    out.n_match = k;
    if (k < 4 || k < job.min_matches) return 0;
    std::vector<double> mbv((size_t) k * 3), muv((size_t) k * 2), mw((size_t) k * 3);
    for (int i = 0; i < k; i++) {
        for (int c = 0; c < 3; c++) mbv[3 * (size_t) i + c] = bv[3 * (size_t) mq[(size_t) i] + c];
        for (int c = 0; c < 2; c++) muv[2 * (size_t) i + c] = (double) unpx[2 * (size_t) mq[(size_t) i] + c];
        for (int c = 0; c < 3; c++) mw[3 * (size_t) i + c] = job.map_wpt[3 * (size_t) mr[(size_t) i] + c];
    }
    // the pose solve of track_pose_collect (track_default.cpp)
    double pose7[7] = {0, 0, 0, 0, 0, 0, 1};
    std::vector<int> outl((size_t) k + 1);
    std::vector<uint8_t> is_out((size_t) k, 0);
    int n_out = 0, ok = 0;
    rc = p3p(k, mbv.data(), mw.data(), job.do_random, pose7, outl.data(), &n_out, &ok);
    if (rc) return rc;
    bool bad_t = false;
    for (int i = 0; i < 3; i++) bad_t = bad_t || std::isinf(pose7[i]) || std::isnan(pose7[i]);
    if (!ok || k - n_out < 5 || bad_t) {
        out.status = 0;
        return 0;
    }
    for (int i = 0; i < n_out; i++) is_out[(size_t) outl[(size_t) i]] = 1;
    std::vector<int> index;
    std::vector<double> uv2, w2;
    for (int i = 0; i < k; i++)
        if (!is_out[(size_t) i]) {
            index.push_back(i);
            uv2.insert(uv2.end(), &muv[2 * (size_t) i], &muv[2 * (size_t) i] + 2);
            w2.insert(w2.end(), &mw[3 * (size_t) i], &mw[3 * (size_t) i] + 3);
        }
    const int n2 = (int) index.size();
    n_out = 0;
    ok = 0;
    rc = pnp(n2, uv2.data(), w2.data(), pose7, outl.data(), &n_out, &ok);
    if (rc) return rc;
    bad_t = false;
    for (int i = 0; i < 3; i++) bad_t = bad_t || std::isinf(pose7[i]) || std::isnan(pose7[i]);
    if (!ok || n2 - n_out < 5 || n_out > 0.5 * n2 || bad_t) {
        out.status = 1;
        return 0;
    }
    for (int i = 0; i < n_out; i++) is_out[(size_t) index[(size_t) outl[(size_t) i]]] = 1;
    out.status = 2;
    std::memcpy(out.pose7, pose7, sizeof(pose7));
    for (int i = 0; i < k; i++) {
        if (is_out[(size_t) i]) continue;
        const size_t q = (size_t) mq[(size_t) i];
        out.px.insert(out.px.end(), &pts[2 * q], &pts[2 * q] + 2);
        out.unpx.insert(out.unpx.end(), &unpx[2 * q], &unpx[2 * q] + 2);
        out.bv.insert(out.bv.end(), &bv[3 * q], &bv[3 * q] + 3);
        out.desc.insert(out.desc.end(), &desc[32 * q], &desc[32 * q] + 32);
        out.mp_id.push_back(job.map_id[mr[(size_t) i]]);
    }
    out.n_inliers = (int) out.mp_id.size();
    return 0;
}

}  // namespace alva_slam
