// Keypoint driver of the drop-in class (include/GaussDePyramid-HIP.h, plain g++): builds the
// pyramid of an n x n LCG image with GaussPyramid_hip::GenerateDoG(), finds its scale-space extrema
// with DetectExtrema(contrast, edge_ratio), and writes GaussPy in the packed [o][s][r][c] layout
// and the returned gdp_keypoint records (16 bytes each, in the order returned).
//     extrema_hip <n> <S> <lcg:SEED> <contrast> <edge_ratio> <pyramid.f32> <keypoints.bin>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "GaussDePyramid-HIP.h"

int main(int argc, char* argv[]) {
    if (argc != 8 || std::string(argv[3]).rfind("lcg:", 0) != 0) {
        std::fprintf(stderr, "usage: see the header of examples/extrema_hip.cpp\n");
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
        const std::vector<gdp_keypoint> kp = g.DetectExtrema(contrast, edge_ratio);
        FILE* f = std::fopen(argv[6], "wb");
        if (!f) return 3;
        int len = n;
        for (int o = 0; o < gdp_octaves_for(n); ++o, len /= 2)
            for (int sc = 0; sc < S + 3; ++sc)
                for (int r = 0; r < len; ++r) std::fwrite(g.GaussPy[o][sc][r], sizeof(float), len, f);
        std::fclose(f);
        f = std::fopen(argv[7], "wb");
        if (!f) return 3;
        if (!kp.empty() && std::fwrite(kp.data(), sizeof(gdp_keypoint), kp.size(), f) != kp.size()) return 3;
        std::fclose(f);
        std::printf("%zu keypoints\n", kp.size());
    }
    for (int i = 0; i < n; ++i) delete[] p[i];
    delete[] p;
    return 0;
}
