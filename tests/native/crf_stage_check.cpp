// crf_stage_check -- crf_stage_clusters (csrc/crf.h), the host transposition of a SimpleCRF window's clusters into the planes and member
// counts the tensor CRF kernels read, checked entry by entry.  Host code only: no device is opened.  Built with the host sanitizers
// and run by tests/test_crf_stage_cpu.py:
//     hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//           -I fast_slic_amd/csrc tests/native/crf_stage_check.cpp -o crf_stage_check
// Every buffer has exactly the size the routine is promised (6 * T * K words, K clusters a frame), so a write or read one past an
// end is the sanitizer's to report.
#include "crf.h"

#include <cstdio>
#include <vector>

static int check(size_t T, size_t K) {
    std::vector<std::vector<fslic_cluster>> frames(T, std::vector<fslic_cluster>(K));
    uint32_t v = (uint32_t)(T * 1000 + K);
    const auto next = [&v] { return v = v * 1664525u + 1013904223u; };
    for (auto& f : frames)
        for (auto& c : f) {
            c.y = (float)(next() >> 8) * 0.25f; c.x = (float)(next() >> 8) * 0.125f;
            c.r = (float)(next() >> 24); c.g = (float)(next() >> 24); c.b = (float)(next() >> 24);
            c.a = -1.0f;                                     // never staged
            c.number = (uint16_t)next();
            c.num_members = next();                          // all 32 bits, the sign bit among them
        }
    frames[T - 1][K - 1].num_members = 0xffffffffu;
    std::vector<float> window(6 * T * K, -2.0f);
    for (size_t w = 0; w < T; w++) fslic::crf_stage_clusters(frames[w].data(), w, T, K, window.data());
    const float* planes = window.data();
    const float* members = window.data() + 5 * T * K;
    int bad = 0;
    for (size_t w = 0; w < T; w++)
        for (size_t i = 0; i < K; i++) {
            const fslic_cluster& c = frames[w][i];
            const float want[5] = {c.y, c.x, c.r, c.g, c.b};
            for (size_t ch = 0; ch < 5; ch++) bad += memcmp(&planes[(w * 5 + ch) * K + i], &want[ch], 4) != 0;
            bad += memcmp(&members[w * K + i], &c.num_members, 4) != 0;
        }
    printf("T=%zu K=%zu: %d of %zu words differ\n", T, K, bad, 6 * T * K);
    return bad;
}

int main() {
    int bad = 0;
    for (size_t T : {1, 3})
        for (size_t K : {1, 63, 65}) bad += check(T, K);
    return bad ? 1 : 0;
}
