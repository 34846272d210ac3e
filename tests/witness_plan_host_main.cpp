// Stand-alone driver of the host planner of the witness completion (csrc/witness_plan.hpp), compiled for the host only with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_witness_plan_host.py and run as a child process.
//
// Input file (text):  curve n_rows n_vars n_pi wide_min_rows / n_pi positions / per row: 5 x 8 selector words (32-bit,
// Montgomery form, little endian) and 3 wire indices.
// Output:  "plan depth max_level_rows n_free n_out n_right n_unused scheduled tuples launches", then per variable
// "kind def_row level", then per scheduled row "row out level".  Every index the schedule holds is checked here against the
// sizes it will be used with on the device.
#include "../zkt-plonk_amd/csrc/witness_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace zkt;

template <class R>
static int run(FILE* f, size_t n_rows, size_t n_vars, size_t n_pi, uint32_t wide_min_rows) {
    std::vector<size_t> pos(n_pi);
    for (size_t& p : pos)
        if (fscanf(f, "%zu", &p) != 1) return 2;
    std::vector<Fe<R>> sel[5];
    std::vector<uint32_t> w[3];
    for (auto& s : sel) s.resize(n_rows);
    for (auto& x : w) x.resize(n_rows);
    for (size_t i = 0; i < n_rows; ++i) {
        for (int k = 0; k < 5; ++k)
            for (int j = 0; j < 8; ++j)
                if (fscanf(f, "%u", &sel[k][i].v[j]) != 1) return 2;
        for (int k = 0; k < 3; ++k)
            if (fscanf(f, "%u", &w[k][i]) != 1) return 2;
    }
    const Fe<R>* selp[5];
    const uint32_t* wp[3];
    for (int k = 0; k < 5; ++k) selp[k] = sel[k].data();
    for (int k = 0; k < 3; ++k) wp[k] = w[k].data();
    WitnessPlan<R> W;
    witness_plan_make<R>(selp, wp, n_rows, n_vars, pos.data(), n_pi, W);
    const std::vector<WpLaunch> launches = witness_plan_split(W.level_start, W.depth, wide_min_rows);

    // what the kernels rely on
    if (W.level_start.size() != (size_t)W.depth + 2 || W.level_start.back() != W.rows.size()) return 3;
    for (size_t l = 0; l + 1 < W.level_start.size(); ++l)
        if (W.level_start[l] > W.level_start[l + 1]) return 3;
    for (const WpRow& r : W.rows) {
        if (r.out >= n_vars || r.row >= n_rows || r.coef >= W.tuples.size()) return 4;
        const bool right = (r.flags & WP_RULE_R) != 0;
        const bool reads0 = wp_flag(r.flags, WP_M) != WP_ZERO || wp_flag(r.flags, WP_L) != WP_ZERO;
        const bool reads1 = right ? wp_flag(r.flags, WP_O) != WP_ZERO : (wp_flag(r.flags, WP_M) != WP_ZERO || wp_flag(r.flags, WP_R) != WP_ZERO);
        if ((reads0 && r.in0 >= n_vars) || (reads1 && r.in1 >= n_vars)) return 5;
        if (reads0 && W.level[r.in0] >= W.level[r.out]) return 6;
        if (reads1 && W.level[r.in1] >= W.level[r.out]) return 6;
    }
    uint32_t next = 1;
    for (const WpLaunch& L : launches) {
        if (L.level0 != next || L.level1 <= L.level0 || (L.wide && L.level1 != L.level0 + 1)) return 7;
        next = L.level1;
    }
    if (!launches.empty() && next != W.depth + 1) return 7;

    printf("plan %u %u %llu %llu %llu %llu %zu %zu %zu\n", W.depth, W.max_level_rows, (unsigned long long)W.n_free,
           (unsigned long long)W.n_out, (unsigned long long)W.n_right, (unsigned long long)W.n_unused, W.rows.size(), W.tuples.size(),
           launches.size());
    for (size_t v = 0; v < n_vars; ++v) printf("%u %u %u\n", (unsigned)W.kind[v], W.def_row[v], W.level[v]);
    for (const WpRow& r : W.rows) printf("%u %u %u\n", r.row, r.out, W.level[r.out]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    int curve = 0;
    size_t n_rows = 0, n_vars = 0, n_pi = 0;
    uint32_t wide = 0;
    if (fscanf(f, "%d %zu %zu %zu %u", &curve, &n_rows, &n_vars, &n_pi, &wide) != 5) return 2;
    const int rc = curve == 0 ? run<Bn254Fr>(f, n_rows, n_vars, n_pi, wide) : run<Bls381Fr>(f, n_rows, n_vars, n_pi, wide);
    fclose(f);
    return rc;
}
