// Stand-alone host program of tests/test_psis_host.py: the plain-C++ part of bipymc_amd/csrc/psis.h -- the kept-set size, the fit, the smoothing
// and the finish of one datum, in the device's own order of operations (a team of 256 lanes, run as loops) -- compiled without a device, once
// plainly and once under the address and undefined-behaviour sanitizers.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I bipymc_amd/csrc tests/psis_host_main.cpp -o psis_host
// Reads commands from the file argv[1], answers one line each on stdout (doubles as C99 hex floats):
//   K <S> <r_eff>                                    -> K <kept>
//   T <n_kept> <n_body> <m_b> <s_b> <n_kept values, ascending>   -> T <k> <sigma> <elpd> <tail_len> <tail_len smoothed log weights, ascending ratio>
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define BPM_VARIANT_NS host_check
#include "psis.h"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: psis_host COMMANDS\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    char cmd = 0;
    int rc = 0;
    while (std::fscanf(f, " %c", &cmd) == 1) {
        if (cmd == 'K') {
            unsigned long long S = 0;
            double r = 0.0;
            if (std::fscanf(f, "%llu %la", &S, &r) != 2) { rc = 3; break; }
            std::printf("K %llu\n", (unsigned long long)bpm::psis_kept(S, r));
        } else if (cmd == 'T') {
            unsigned n_kept = 0;
            unsigned long long n_body = 0;
            double mb = 0.0, sb = 0.0;
            if (std::fscanf(f, "%u %llu %la %la", &n_kept, &n_body, &mb, &sb) != 4 || n_kept == 0) { rc = 3; break; }
            std::vector<double> tail(n_kept), ws((size_t)bpm::psis_work(n_kept)), sm(n_kept), red(bpm::PSIS_THREADS);
            bool ok = true;
            for (unsigned j = 0; j < n_kept; ++j) ok = ok && std::fscanf(f, "%la", &tail[j]) == 1;
            if (!ok) { rc = 3; break; }
            bpm::PsisTeam tm;
            tm.red = red.data();
            const bpm::PsisResult r = bpm::psis_datum(tm, tail.data(), n_kept, n_body, mb, sb, ws.data(), sm.data());
            std::printf("T %a %a %a %llu", r.k, r.sigma, r.elpd, (unsigned long long)r.tail_len);
            for (uint64_t j = 0; j < r.tail_len; ++j) std::printf(" %a", sm[(size_t)j]);
            std::printf("\n");
        } else { rc = 3; break; }
    }
    std::fclose(f);
    if (rc) std::fprintf(stderr, "psis_host: malformed command file\n");
    return rc;
}
