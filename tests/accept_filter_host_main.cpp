// Stand-alone host program of tests/test_accept_filter_host.py: bipymc_amd/csrc/accept_test.h in its host flavour (exp2f for the device's
// v_exp_f32) against the plain formula of the accept test, written out here a second time.  Prints one line of counts.
//   g++ -O2 -std=c++17 -ffp-contract=off -I bipymc_amd/csrc tests/accept_filter_host_main.cpp -o accept_filter_host && ./accept_filter_host
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "accept_test.h"

namespace {

struct Plain { bool accepted, is_nan; double alpha; };
Plain plain(double d, double u) {
    double alpha = std::exp(d);
    const bool is_nan = alpha != alpha;
    alpha = std::fmin(1.0, alpha);
    alpha = std::fmax(0.0, alpha);
    return {!is_nan && (u < alpha), is_nan, alpha};
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double u53() { return (double)(next_u64() >> 11) * 0x1p-53; }

struct Tally { long long n = 0, diff_accept = 0, diff_nan = 0, exact = 0; };
void one(double d, double u, Tally& t) {
    const Plain p = plain(d, u);
    bool nan_f = false, nan_t = false, yes = false, ask = false;
    bpm::accept_filter(d, u, &yes, &ask, &nan_f);
    const bool acc = bpm::accept_test(d, u, &nan_t);
    ++t.n;
    t.diff_accept += acc != p.accepted;
    t.diff_nan += (nan_t != p.is_nan) || (nan_f != p.is_nan);
    t.exact += ask;
    if ((acc != p.accepted || nan_t != p.is_nan) && t.diff_accept + t.diff_nan <= 10)
        std::printf("# differs: d=%a u=%a plain accepted=%d nan=%d, accept_test accepted=%d nan=%d (filter yes=%d ask=%d)\n", d, u, (int)p.accepted,
                    (int)p.is_nan, (int)acc, (int)nan_t, (int)yes, (int)ask);
}

// u within +-2 ulp of the clamped exp(d)
void adversarial(double d, Tally& t) {
    const double a = plain(d, 0.0).alpha;
    if (a != a) { one(d, 0.5, t); return; }
    const double inf = std::numeric_limits<double>::infinity();
    double lo = a, hi = a;
    one(d, a, t);
    for (int k = 0; k < 2; ++k) {
        lo = std::nextafter(lo, -inf); hi = std::nextafter(hi, inf);
        one(d, lo, t); one(d, hi, t);
    }
}

void fixed_u(double d, Tally& t) {
    one(d, 0.0, t); one(d, 0x1p-53, t); one(d, 1.0 - 0x1p-53, t);
}

}   // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double dlo = bpm::ACCEPT_D_LO;
    std::vector<double> ds = {0.0, -0.0, 1e-300, -1e-300, dlo, std::nextafter(dlo, -inf), std::nextafter(dlo, inf), -745.0, -746.0, -1e300, inf, -inf, nan};
    const size_t n_special = ds.size();
    for (int i = 0; i < 1000000; ++i) ds.push_back(-45.0 + 46.0 * u53());
    Tally plain_u, adv;
    for (size_t i = 0; i < ds.size(); ++i) {
        const double d = ds[i];
        fixed_u(d, plain_u);
        const int n_rand = i < n_special ? 1000 : 1;
        for (int k = 0; k < n_rand; ++k) one(d, u53(), plain_u);
        adversarial(d, adv);
    }
    std::printf("n_random_u %lld diff_accept %lld diff_nan %lld exact %lld\n", plain_u.n, plain_u.diff_accept, plain_u.diff_nan, plain_u.exact);
    std::printf("n_adversarial %lld diff_accept %lld diff_nan %lld exact %lld\n", adv.n, adv.diff_accept, adv.diff_nan, adv.exact);
    std::printf("exp_d_lo_below_u_min %d\n", (int)(std::exp(dlo) < bpm::ACCEPT_U_MIN));
    return 0;
}
