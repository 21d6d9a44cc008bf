// Stand-alone driver of arl_goat_item_sample for tests/test_goat_cpu.py: built together with arlib_amd/csrc/arl_host.cpp under
// -fsanitize=address,undefined and run as a program of its own (nothing is loaded into python).
//
//   goat_sample_main IN OUT
// IN : int64 U, I, nnz, T, F, n_k, calls, seed | int64 rowptr[U + 1] | int32 items[nnz] | double int_num[I] | int32 targets[T] | int64 k[n_k]
//      | double O_u, O_i
// OUT: per k, per call: int32 I_s[F][int(0.3 k)] | int32 I_f[F][k - int(0.3 k)] | uint8 real[F][k] | int32 user | uint32 mt[625]
// Every buffer has exactly the size the header of the library asks for, so a write past one of them is the sanitizer's to see.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "arlib_amd.h"

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(2); }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int64_t> h = take<int64_t>(in, 8);
    const int64_t U = h[0], I = h[1], nnz = h[2], T = h[3], F = h[4], n_k = h[5], calls = h[6];
    const std::vector<int64_t> rowptr = take<int64_t>(in, (size_t)U + 1);
    const std::vector<int32_t> items = take<int32_t>(in, (size_t)nnz);
    const std::vector<double> int_num = take<double>(in, (size_t)I);
    const std::vector<int32_t> targets = take<int32_t>(in, (size_t)T);
    const std::vector<int64_t> ks = take<int64_t>(in, (size_t)n_k);
    const std::vector<double> o = take<double>(in, 2);
    for (int64_t q = 0; q < n_k; ++q) {
        const int64_t k = ks[(size_t)q], s = (int64_t)((double)k * 0.3);
        std::vector<uint32_t> mt(625);
        const uint32_t key = (uint32_t)h[7];
        if (arl_mt_seed(mt.data(), &key, 1) != ARL_OK) return 3;
        for (int64_t c = 0; c < calls; ++c) {
            std::vector<int32_t> I_s((size_t)(F * s)), I_f((size_t)(F * (k - s))), user(1);
            std::vector<uint8_t> real((size_t)(F * k));
            std::vector<int32_t> scratch((size_t)arl_goat_item_sample_scratch_words(I, k, T));
            const int rc = arl_goat_item_sample(mt.data(), rowptr.data(), items.data(), U, I, int_num.data(), targets.data(), T, F, k, o[0] * (double)I,
                                                (int64_t)(o[1] * (double)U), I_s.data(), I_f.data(), real.data(), user.data(), scratch.data());
            if (rc != ARL_OK) { fprintf(stderr, "arl_goat_item_sample: %d\n", rc); return 4; }
            put(out, I_s); put(out, I_f); put(out, real); put(out, user); put(out, mt);
        }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
