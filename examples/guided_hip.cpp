// Guided matching driver of the drop-in class (include/GaussDePyramid-HIP.h, plain g++): two n x n
// LCG images of the same seed, the second one moved `shift` columns to the right (cyclically).  Both
// get the whole chain on the device after gdp_build_gaussian — DetectExtrema(),
// RefineKeypoints(contrast, edge_ratio), OrientKeypoints(), DescribeKeypoints() — and the first is
// matched against the second with GuidedMatch() under the translation by (shift, 0): every query only
// against the records within `radius` pixels of where the model puts it.  Prints the count and the
// first eight records.
//     guided_hip <n> <S> <lcg:SEED> <shift> <contrast> <edge_ratio> <radius> <ratio> <unique 0|1>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
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

int main(int argc, char* argv[]) {
    if (argc != 10 || std::string(argv[3]).rfind("lcg:", 0) != 0) {
        std::fprintf(stderr, "usage: see the header of examples/guided_hip.cpp\n");
        return 2;
    }
    const int n = std::atoi(argv[1]);
    const int S = std::atoi(argv[2]);
    uint32_t s = (uint32_t)std::strtoul(argv[3] + 4, nullptr, 0);
    const int shift = std::atoi(argv[4]);
    const float contrast = std::strtof(argv[5], nullptr);
    const float edge_ratio = std::strtof(argv[6], nullptr);
    const float radius = std::strtof(argv[7], nullptr);
    const float ratio = std::strtof(argv[8], nullptr);
    const bool unique = std::atoi(argv[9]) != 0;
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
        size_t described[2] = {0, 0};
        int k = 0;
        for (ScaleSpace* g : {&a, &b}) {
            g->mirror_host = false;  // the device pyramid is what the chain reads
            g->Build();
            g->DetectExtrema();
            g->RefineKeypoints(contrast, edge_ratio);
            g->OrientKeypoints();
            described[k++] = g->DescribeKeypoints().size();
        }
        const float h[9] = {1.0f, 0.0f, (float)shift, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};  // (x, y) -> (x + shift, y)
        const std::vector<gdp_match_record> m = a.GuidedMatch(b, h, radius, ratio, 0xffffffffu, unique);
        std::printf("%zu guided matches of %zu x %zu\n", m.size(), described[0], described[1]);
        for (size_t i = 0; i < m.size() && i < 8; ++i)
            std::printf("query %u train %u distance %u second %u (%.4f, %.4f) -> (%.4f, %.4f)\n", m[i].query, m[i].train,
                        m[i].distance, m[i].second, m[i].qx, m[i].qy, m[i].tx, m[i].ty);
    }
    for (int i = 0; i < n; ++i) {
        delete[] p[i];
        delete[] q[i];
    }
    delete[] p;
    delete[] q;
    return 0;
}
