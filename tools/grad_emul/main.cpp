#include "ecorr.h"
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>
static std::vector<float> rd(const std::string& p) {
    FILE* f = fopen(p.c_str(), "rb"); if (!f) { perror(p.c_str()); exit(2); }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<float> v(n / 4); if (fread(v.data(), 4, v.size(), f) != v.size()) exit(2); fclose(f); return v;
}
static void wr(const std::string& p, const float* d, size_t n) { FILE* f = fopen(p.c_str(), "wb"); fwrite(d, 4, n, f); fclose(f); }
int main(int argc, char** argv) {
    std::string dir = argv[1];
    int B, D, H, W, L, r, nl, q;
    FILE* m = fopen((dir + "/meta.txt").c_str(), "r");
    if (fscanf(m, "%d %d %d %d %d %d %d %d", &B, &D, &H, &W, &L, &r, &nl, &q) != 8) return 2;
    fclose(m);
    std::vector<int> h(L), w(L); std::vector<int64_t> off(L + 1);
    if (ecorr_pyramid_layout((int64_t)B * q, H, W, L, h.data(), w.data(), off.data())) return 3;
    // exact-size heap buffers: ASan flags any access outside
    std::vector<float> G(off[L], 0.f), f1 = rd(dir + "/f1.bin"), f2 = rd(dir + "/f2.bin");
    for (int i = 0; i < nl; ++i) {
        auto c = rd(dir + "/coords" + std::to_string(i) + ".bin"), g = rd(dir + "/go" + std::to_string(i) + ".bin");
        int st = ecorr_lookup_backward(g.data(), c.data(), B, H, W, q, L, r, G.data(), nullptr);
        if (st) { printf("lookup_backward status %d\n", st); return 4; }
    }
    wr(dir + "/G.bin", G.data(), G.size());
    std::vector<float> g1((size_t)B * D * q, NAN), g2((size_t)B * D * H * W, NAN);
    int st = ecorr_build_backward(G.data(), f1.data(), f2.data(), B, D, H, W, q, L, g1.data(), g2.data(), nullptr);
    if (st) { printf("build_backward status %d\n", st); return 5; }
    wr(dir + "/g1.bin", g1.data(), g1.size()); wr(dir + "/g2.bin", g2.data(), g2.size());
    printf("ok %s\n", dir.c_str());
    return 0;
}
