// Least-squares refit driver of the drop-in class (include/GaussDePyramid-HIP.h, plain g++): two
// n x n LCG images of the same seed, the second one moved `shift` columns to the right (cyclically).
// Both get the whole chain on the device after gdp_build_gaussian — DetectExtrema(),
// RefineKeypoints(contrast, edge_ratio), OrientKeypoints(), DescribeKeypoints() — the first is
// matched against the second with MatchDescriptors(ratio, no cap, mutual); FitHomography() fits the
// matches (sorted by their coordinates, so the result does not depend on the device order) and
// RefitHomography() fits them again and refits the model over its inliers.  Prints the model record
// before and after, and the refit record.
//     refit_hip <n> <S> <lcg:SEED> <shift> <contrast> <edge_ratio> <ratio> <hypotheses> <seed> <threshold> <rounds> <refit threshold>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "GaussDePyramid-HIP.h"

// the class plus gdp_build_gaussian on its context: a real scale space, which is what SIFT describes
struct ScaleSpace : GaussPyramid_hip {
    ScaleSpace(int** img, int n, int S) : GaussPyramid_hip(img, n, S) {}
    void Build() {  // the constructor uploaded the image
        if (gdp_build_gaussian(ctx_, nullptr) != GDP_OK || gdp_sync(ctx_) != GDP_OK) {
            std::fprintf(stderr, "gdp_build_gaussian failed: %s\n", gdp_last_error(ctx_));
            std::abort();
        }
    }
};

static void print_model(const char* name, const gdp_homography& H, size_t inliers, size_t matches) {
    std::printf("%s: %zu inliers of %zu matches\n", name, inliers, matches);
    std::printf("hypothesis %u inliers %u matches %u sample %u %u %u %u\n", H.hypothesis, H.inliers, H.matches, H.sample[0], H.sample[1],
                H.sample[2], H.sample[3]);
    for (int r = 0; r < 3; ++r) {  // the floats' bits, so that the comparison is exact
        uint32_t w[3];
        std::memcpy(w, H.h + 3 * r, sizeof w);
        std::printf("h %08x %08x %08x  (%.9g %.9g %.9g)\n", w[0], w[1], w[2], H.h[3 * r], H.h[3 * r + 1], H.h[3 * r + 2]);
    }
}

int main(int argc, char* argv[]) {
    if (argc != 13 || std::string(argv[3]).rfind("lcg:", 0) != 0) {
        std::fprintf(stderr, "usage: see the header of examples/refit_hip.cpp\n");
        return 2;
    }
    const int n = std::atoi(argv[1]);
    const int S = std::atoi(argv[2]);
    uint32_t s = (uint32_t)std::strtoul(argv[3] + 4, nullptr, 0);
    const int shift = std::atoi(argv[4]);
    const float contrast = std::strtof(argv[5], nullptr);
    const float edge_ratio = std::strtof(argv[6], nullptr);
    const float ratio = std::strtof(argv[7], nullptr);
    const uint32_t hypotheses = (uint32_t)std::strtoul(argv[8], nullptr, 0);
    const uint32_t seed = (uint32_t)std::strtoul(argv[9], nullptr, 0);
    const float threshold = std::strtof(argv[10], nullptr);
    const uint32_t rounds = (uint32_t)std::strtoul(argv[11], nullptr, 0);
    const float refit_threshold = std::strtof(argv[12], nullptr);
    if (n <= 0 || shift < 0 || shift >= n) return 2;
    int** p = new int*[n];
    int** q = new int*[n];
    for (int i = 0; i < n; ++i) {
        p[i] = new int[n];
        q[i] = new int[n];
        for (int j = 0; j < n; ++j) {  // SURVEY.md Appendix A LCG, row-major
            s = s * 1664525u + 1013904223u;
            p[i][j] = (int)(s >> 24);
        }
        for (int j = 0; j < n; ++j) q[i][(j + shift) % n] = p[i][j];
    }
    {
        ScaleSpace a(p, n, S), b(q, n, S);
        for (ScaleSpace* g : {&a, &b}) {
            g->mirror_host = false;  // the device pyramid is what the chain reads
            g->Build();
            g->DetectExtrema();
            g->RefineKeypoints(contrast, edge_ratio);
            g->OrientKeypoints();
            g->DescribeKeypoints();
        }
        std::vector<gdp_match_record> m = a.MatchDescriptors(b, ratio, 0xffffffffu, true);
        // `query` and `train` name the described lists in device order, which may differ from run to run:
        // the coordinates do not, and they are all the fit reads
        std::sort(m.begin(), m.end(), [](const gdp_match_record& p, const gdp_match_record& q) {
            return std::tie(p.qx, p.qy, p.tx, p.ty, p.distance, p.second) < std::tie(q.qx, q.qy, q.tx, q.ty, q.distance, q.second);
        });
        std::vector<gdp_match_record> inliers;
        const gdp_homography before = a.FitHomography(m, &inliers, hypotheses, seed, threshold, 4);
        print_model("fit", before, inliers.size(), m.size());
        gdp_refit_record rec;
        const gdp_homography after = a.RefitHomography(m, &inliers, &rec, rounds, refit_threshold, hypotheses, seed, threshold, 4);
        print_model("refit", after, inliers.size(), m.size());
        uint32_t w[24];  // the whole record, bit for bit
        static_assert(sizeof w == sizeof rec, "96 bytes");
        std::memcpy(w, &rec, sizeof w);
        std::printf("record");
        for (uint32_t v : w) std::printf(" %08x", v);
        std::printf("\nrounds %u accepted %u used %u skipped %u count %u -> %u status %u\n", rec.rounds, rec.accepted, rec.used, rec.skipped,
                    rec.count_before, rec.count_after, rec.status);
    }
    for (int i = 0; i < n; ++i) {
        delete[] p[i];
        delete[] q[i];
    }
    delete[] p;
    delete[] q;
    return 0;
}
