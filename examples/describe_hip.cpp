// SIFT descriptor driver of the drop-in class (include/GaussDePyramid-HIP.h, plain g++): builds the
// pyramid of an n x n LCG image with GaussPyramid_hip::GenerateDoG(), finds its scale-space extrema
// with DetectExtrema(), localises them with RefineKeypoints(contrast, edge_ratio), assigns their
// orientations with OrientKeypoints(), computes their descriptors with DescribeKeypoints() and
// prints the counts and the first records, each with its 128 descriptor bytes in hexadecimal.
//     describe_hip <n> <S> <lcg:SEED> <contrast> <edge_ratio>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "GaussDePyramid-HIP.h"

int main(int argc, char* argv[]) {
    if (argc != 6 || std::string(argv[3]).rfind("lcg:", 0) != 0) {
        std::fprintf(stderr, "usage: see the header of examples/describe_hip.cpp\n");
        return 2;
    }
    const int n = std::atoi(argv[1]);
    const int S = std::atoi(argv[2]);
    uint32_t s = (uint32_t)std::strtoul(argv[3] + 4, nullptr, 0);
    const float contrast = std::strtof(argv[4], nullptr);
    const float edge_ratio = std::strtof(argv[5], nullptr);
    int** p = new int*[n];
    for (int i = 0; i < n; ++i) {
        p[i] = new int[n];
        for (int j = 0; j < n; ++j) {  // SURVEY.md Appendix A LCG, row-major
            s = s * 1664525u + 1013904223u;
            p[i][j] = (int)(s >> 24);
        }
    }
    {
        GaussPyramid_hip g(p, n, S);
        g.GenerateDoG();
        const std::vector<gdp_keypoint> kp = g.DetectExtrema();
        const std::vector<gdp_keypoint_refined> rf = g.RefineKeypoints(contrast, edge_ratio);
        const std::vector<gdp_keypoint_oriented> ok = g.OrientKeypoints();
        const std::vector<gdp_keypoint_described> de = g.DescribeKeypoints();
        std::printf("%zu keypoints, %zu refined, %zu oriented, %zu described\n", kp.size(), rf.size(), ok.size(), de.size());
        for (size_t i = 0; i < de.size() && i < 8; ++i) {
            const gdp_keypoint_described& k = de[i];
            std::printf("octave %d scale %d sample (%d, %d) angle %.4f bin %u desc ", (int)k.octave, (int)k.scale, k.row, k.col,
                        k.angle, k.bin);
            for (int t = 0; t < 128; ++t) std::printf("%02x", (unsigned)k.desc[t]);
            std::printf("\n");
        }
    }
    for (int i = 0; i < n; ++i) delete[] p[i];
    delete[] p;
    return 0;
}
