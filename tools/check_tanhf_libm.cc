// check_tanhf_libm.cc -- holds csrc/tanhf_libm.h (the soft-cap's tanhf of the CPU-exact mixed-cache attention kernel) on the host, bit for bit, against
//   check_tanhf_libm --file PAIRS   recorded values: a raw file of f32 pairs (x, tanhf(x)), what tests/test_tanhf_libm_cpu.py writes from tests/golden/tanhf_libm.npz
//   check_tanhf_libm [STRIDE]       THIS host's C library: every STRIDE-th f32 bit pattern, all exponents and both signs (default 1: all 2^32 of them, a few
//                                   seconds on 8 threads).  Only meaningful where that library has the fdlibm form (the GNU C library up to 2.40).
//   c++ -O2 -ffp-contract=off -std=c++17 -pthread -Illama.cpp.dsp_amd/csrc tools/check_tanhf_libm.cc -o check_tanhf_libm -lm
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "tanhf_libm.h"

#include <string.h>

static int check_file(const char * path) {
    FILE * f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); return 2; }
    float p[2];
    unsigned long long n = 0, bad = 0;
    while (fread(p, sizeof(float), 2, f) == 2) {
        const float m = mi355q::tanhf_libm(p[0]);
        if (mi355q::tl_bits(m) != mi355q::tl_bits(p[1]) && !(m != m && p[1] != p[1])) { if (bad < 3) printf("x = %a: recorded %a, tanhf_libm %a\n", p[0], p[1], m); ++bad; }
        ++n;
    }
    fclose(f);
    printf("checked %llu values, %llu differ\n", n, bad);
    return bad != 0 || n == 0;
}

int main(int argc, char ** argv) {
    if (argc > 2 && !strcmp(argv[1], "--file")) return check_file(argv[2]);
    const uint64_t stride = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int n_threads = 8;
    std::atomic<uint64_t> bad{0}, n{0};
    std::vector<std::thread> th;
    for (int w = 0; w < n_threads; ++w) th.emplace_back([&, w] {
        uint64_t b = 0, c = 0;
        for (uint64_t u = w * stride; u < 0x100000000ull; u += n_threads * stride) {
            const float x = mi355q::tl_float((uint32_t) u);
            const float a = tanhf(x), m = mi355q::tanhf_libm(x);
            if (mi355q::tl_bits(a) != mi355q::tl_bits(m) && !(a != a && m != m)) { if (b < 3) printf("x = %a: C library %a, tanhf_libm %a\n", x, a, m); ++b; }
            ++c;
        }
        bad += b; n += c; });
    for (auto & t : th) t.join();
    printf("checked %llu values, %llu differ\n", (unsigned long long) n.load(), (unsigned long long) bad.load());
    return bad.load() != 0;
}
