// For orientation beside `colorid dists` (profiles/dists_summary.md): the same two A x A matrices by a plain C++ loop on 16 host threads.
// Reads a table in the form of PREFIX.raw.tsv, numbers the alleles as the CLI does, and times differ / compared over every ordered pair
// (the rectangle cid_dists_rows computes; no use of symmetry).  Prints the time and a checksum of both matrices; writes nothing.
//   g++ -O3 -march=native -std=c++17 -pthread -o tools/bin/dists_cpu_loop tools/dists_cpu_loop.cpp ;  tools/bin/dists_cpu_loop TABLE [threads]
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: dists_cpu_loop TABLE [threads]\n"); return 2; }
    const int n_threads = argc > 2 ? atoi(argv[2]) : 16;
    std::ifstream in(argv[1]);
    std::string line;
    if (!std::getline(in, line)) { fprintf(stderr, "no header\n"); return 1; }
    size_t L = 0;
    for (char ch : line) L += ch == '\t';
    std::vector<std::unordered_map<std::string, uint32_t>> maps(L);
    std::vector<uint32_t> codes;
    size_t A = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        size_t p = line.find('\t'), l = 0;
        while (p != std::string::npos && l < L) {
            const size_t e = line.find('\t', p + 1);
            const std::string cell = line.substr(p + 1, e == std::string::npos ? std::string::npos : e - p - 1);
            uint32_t code = 0;
            if (!cell.empty() && cell != "NA") code = maps[l].emplace(cell, (uint32_t)maps[l].size() + 1).first->second;
            codes.push_back(code);
            ++l;
            p = e;
        }
        if (l != L) { fprintf(stderr, "line of %zu cells, header of %zu\n", l, L); return 1; }
        ++A;
    }
    std::vector<uint64_t> sum_d(n_threads, 0), sum_c(n_threads, 0);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (int t = 0; t < n_threads; ++t)
        pool.emplace_back([&, t] {
            uint64_t sd = 0, sc = 0;
            for (size_t i = t; i < A; i += n_threads) {
                const uint32_t *a = &codes[i * L];
                for (size_t j = 0; j < A; ++j) {
                    const uint32_t *b = &codes[j * L];
                    uint32_t compared = 0, differ = 0;
                    for (size_t l = 0; l < L; ++l) {
                        const uint32_t both = (a[l] != 0) & (b[l] != 0);
                        compared += both;
                        differ += both & (a[l] != b[l]);
                    }
                    sd += differ;
                    sc += compared;
                }
            }
            sum_d[t] = sd;
            sum_c[t] = sc;
        });
    for (auto &th : pool) th.join();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    uint64_t sd = 0, sc = 0;
    for (int t = 0; t < n_threads; ++t) { sd += sum_d[t]; sc += sum_c[t]; }
    printf("dists_cpu_loop: %zu accessions x %zu loci, %d threads: %.0f ms for both matrices (sum differ %llu, sum compared %llu)\n", A, L, n_threads, ms,
           (unsigned long long)sd, (unsigned long long)sc);
    return 0;
}
