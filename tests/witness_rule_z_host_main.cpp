// Stand-alone driver of the host planner of the witness completion under a choice of rules (csrc/witness_plan.hpp) and of a
// host evaluation of the schedule it makes -- records, flags and tuples read as the kernels of csrc/witness_plan.hip read them,
// through the same ZKT_HD field arithmetic.  Compiled for the host only with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_witness_rule_z_host.py and run as a child process.
//
// Input file (text):  curve n_rows n_vars n_pi rules n_witnesses / n_pi positions / per row: 5 x 8 selector words (32-bit,
// Montgomery form, little endian) and 3 wire indices / per witness: n_vars x 8 words.
// Output:  "plan depth max_level_rows n_free n_out n_right n_unused n_pairs scheduled tuples", per variable
// "kind def_row level", per scheduled record "row out out2 level", then per witness n_vars lines of 8 words: the completed map.
#include "../zkt-plonk_amd/csrc/witness_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace zkt;

template <class R>
static void term(Fe<R>& acc, uint32_t flag, const Fe<R>& t, const Fe<R>& x) {
    if (flag == WP_ONE) acc = fe_add<R>(acc, x);
    else if (flag == WP_MINUS_ONE) acc = fe_sub<R>(acc, x);
    else if (flag == WP_GEN) acc = fe_add<R>(acc, fe_mul<R>(t, x));
}

// one record on the map x, as wp_row
template <class R>
static void eval(const WitnessPlan<R>& W, const WpRow& r, std::vector<Fe<R>>& x) {
    const Fe<R>* const t = W.tuples[r.coef].t;
    uint32_t f[5];
    for (int k = 0; k < 5; ++k) f[k] = wp_flag(r.flags, k);
    const Fe<R> one = fe_one<R>();
    Fe<R> v = fe_zero<R>();
    if (r.flags & WP_RULE_Z) {
        Fe<R> a = fe_zero<R>(), z = fe_zero<R>();
        if (f[WP_L] != WP_ZERO) a = x.at(r.in0);
        if (fe_is_zero<R>(a)) term<R>(z, f[WP_O], t[WP_O], one);
        else if (f[WP_M] != WP_ZERO) term<R>(v, f[WP_M], t[WP_M], fe_inv_host<R>(a));
        x.at(r.out2) = z;
    } else if (!(r.flags & WP_RULE_R)) {
        Fe<R> a = fe_zero<R>(), b = fe_zero<R>();
        if (f[WP_M] != WP_ZERO || f[WP_L] != WP_ZERO) a = x.at(r.in0);
        if (f[WP_M] != WP_ZERO || f[WP_R] != WP_ZERO) b = x.at(r.in1);
        term<R>(v, f[WP_C], t[WP_C], one);
        if (f[WP_M] != WP_ZERO) term<R>(v, f[WP_M], t[WP_M], fe_mul<R>(a, b));
        term<R>(v, f[WP_L], t[WP_L], a);
        term<R>(v, f[WP_R], t[WP_R], b);
    } else {
        Fe<R> a = fe_zero<R>(), c = fe_zero<R>(), den = fe_zero<R>();
        if (f[WP_M] != WP_ZERO || f[WP_L] != WP_ZERO) a = x.at(r.in0);
        if (f[WP_O] != WP_ZERO) c = x.at(r.in1);
        term<R>(den, f[WP_R], t[WP_R], one);
        term<R>(den, f[WP_M], t[WP_M], a);
        if (!fe_is_zero<R>(den)) {
            term<R>(v, f[WP_C], t[WP_C], one);
            term<R>(v, f[WP_L], t[WP_L], a);
            term<R>(v, f[WP_O], t[WP_O], c);
            v = fe_mul<R>(v, fe_inv_host<R>(den));
        }
    }
    x.at(r.out) = v;
}

template <class R>
static int run(FILE* f, size_t n_rows, size_t n_vars, size_t n_pi, uint32_t rules, size_t n_wit) {
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
    witness_plan_make<R>(selp, wp, n_rows, n_vars, pos.data(), n_pi, W, rules);

    // what the kernels rely on
    if (W.level_start.size() != (size_t)W.depth + 2 || W.level_start.back() != W.rows.size()) return 3;
    size_t pairs = 0;
    for (const WpRow& r : W.rows) {
        if (r.out >= n_vars || r.row >= n_rows || r.coef >= W.tuples.size()) return 4;
        if (r.flags & WP_RULE_Z) {
            ++pairs;
            if ((r.flags & WP_RULE_R) || r.out2 >= n_vars || r.out2 == r.out || r.row + 1 >= n_rows) return 4;
            if (wp_flag(r.flags, WP_L) != WP_ZERO && (r.in0 >= n_vars || W.level[r.in0] >= W.level[r.out])) return 5;
            if (W.level[r.out] != W.level[r.out2] || W.kind[r.out] != WP_ZINV || W.kind[r.out2] != WP_ZFLAG) return 6;
        }
    }
    if (pairs != W.n_pairs || (!(rules & WP_RULES_IS_ZERO) && pairs)) return 7;

    printf("plan %u %u %llu %llu %llu %llu %llu %zu %zu\n", W.depth, W.max_level_rows, (unsigned long long)W.n_free,
           (unsigned long long)W.n_out, (unsigned long long)W.n_right, (unsigned long long)W.n_unused, (unsigned long long)W.n_pairs,
           W.rows.size(), W.tuples.size());
    for (size_t v = 0; v < n_vars; ++v) printf("%u %u %u\n", (unsigned)W.kind[v], W.def_row[v], W.level[v]);
    for (const WpRow& r : W.rows) printf("%u %u %u %u\n", r.row, r.out, (r.flags & WP_RULE_Z) ? r.out2 : WP_VAR_ZERO, W.level[r.out]);
    for (size_t k = 0; k < n_wit; ++k) {
        std::vector<Fe<R>> x(n_vars);
        for (Fe<R>& e : x)
            for (int j = 0; j < 8; ++j)
                if (fscanf(f, "%u", &e.v[j]) != 1) return 2;
        for (const WpRow& r : W.rows) eval<R>(W, r, x);   // the schedule's order: by level
        for (const Fe<R>& e : x) printf("%u %u %u %u %u %u %u %u\n", e.v[0], e.v[1], e.v[2], e.v[3], e.v[4], e.v[5], e.v[6], e.v[7]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    int curve = 0;
    size_t n_rows = 0, n_vars = 0, n_pi = 0, n_wit = 0;
    uint32_t rules = 0;
    if (fscanf(f, "%d %zu %zu %zu %u %zu", &curve, &n_rows, &n_vars, &n_pi, &rules, &n_wit) != 6) return 2;
    const int rc = curve == 0 ? run<Bn254Fr>(f, n_rows, n_vars, n_pi, rules, n_wit) : run<Bls381Fr>(f, n_rows, n_vars, n_pi, rules, n_wit);
    fclose(f);
    return rc;
}
