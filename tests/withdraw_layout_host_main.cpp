// Stand-alone driver of the host planner of the withdraw circuit (csrc/withdraw_layout.hpp), compiled for the host only with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_withdraw_layout_host.py and run as a child process.
//
// Input file (text):  curve width half_full partial inputs height / the round constants, the MDS entries and the domain
// tag as 8 words each (32-bit, Montgomery form, little endian).
// Output:  "shape n_gates n_vars n_hashes per_hash n_pi", the public-input positions on one line, per hash call
// "base arity in0 in1 in2", then per row the six selectors as 8 words each and the three wires.  Every index the plan
// holds is checked here against the sizes it is used with on the device.
#include "../zkt-plonk_amd/csrc/withdraw_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace zkt;
namespace wd = zkt::withdraw;

template <class R>
static bool read_fe(FILE* f, Fe<R>& x) {
    for (int j = 0; j < 8; ++j)
        if (fscanf(f, "%u", &x.v[j]) != 1) return false;
    return true;
}

template <class R>
static int run(FILE* f, const wd::Shape& s) {
    std::vector<Fe<R>> rc((size_t)(2 * s.half_full + s.partial) * s.width), mds((size_t)s.width * s.width);
    Fe<R> tag;
    for (auto& x : rc)
        if (!read_fe<R>(f, x)) return 2;
    for (auto& x : mds)
        if (!read_fe<R>(f, x)) return 2;
    if (!read_fe<R>(f, tag)) return 2;
    wd::Plan pl;
    if (!wd::plan_make(s, pl)) return 3;
    wd::Template<R> t[4];
    for (int a = 1; a <= 3; ++a) {
        wd::template_make<R>(s, rc.data(), mds.data(), tag, a, t[a]);
        for (int q = 0; q < 5; ++q)
            if (t[a].sel[q].size() != s.P) return 4;
        for (int x = 0; x < 3; ++x) {
            if (t[a].w[x].size() != s.P) return 4;
            for (uint32_t ref : t[a].w[x]) {               // what the stamping kernel relies on
                if (ref == wd::REF_ZERO) continue;
                if (ref & wd::REF_INPUT) {
                    if ((int)(ref & ~wd::REF_INPUT) >= a) return 5;
                } else if (ref >= s.P) {
                    return 5;
                }
            }
        }
    }
    for (const wd::HashCall& h : pl.calls) {
        if (h.arity < 1 || h.arity > 3 || (uint64_t)h.row + s.P > s.n_gates || (uint64_t)h.base + s.P > s.n_vars) return 6;
        for (uint32_t k = 0; k < h.arity; ++k)
            if (h.in[k] >= s.n_vars) return 6;
    }
    for (const wd::GlueRow& g : pl.glue) {
        if (g.row >= s.n_gates) return 7;
        for (int x = 0; x < 3; ++x)
            if (g.w[x] != wd::REF_ZERO && g.w[x] >= s.n_vars) return 7;
        for (int q = 0; q < 6; ++q)
            if (g.q[q] >= wd::G_COUNT) return 7;
    }
    std::vector<Fe<R>> sel[6];
    std::vector<uint32_t> w[3];
    Fe<R>* selp[6];
    uint32_t* wp[3];
    for (int q = 0; q < 6; ++q) {
        sel[q].resize((size_t)s.n_gates);
        selp[q] = sel[q].data();
    }
    for (int x = 0; x < 3; ++x) {
        w[x].assign((size_t)s.n_gates, 0xDEADBEEFu);
        wp[x] = w[x].data();
    }
    wd::expand_host<R>(pl, t, selp, wp);
    printf("shape %llu %llu %u %u %u\n", (unsigned long long)s.n_gates, (unsigned long long)s.n_vars, s.n_hashes, s.P, s.n_pi);
    for (size_t p : pl.pi_pos) printf("%zu ", p);
    printf("\n");
    for (const wd::HashCall& h : pl.calls) printf("%u %u %u %u %u\n", h.base, h.arity, h.in[0], h.in[1], h.in[2]);
    for (size_t i = 0; i < s.n_gates; ++i) {
        for (int q = 0; q < 6; ++q)
            for (int j = 0; j < 8; ++j) printf("%u ", sel[q][i].v[j]);
        printf("%u %u %u\n", w[0][i], w[1][i], w[2][i]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    int curve = 0, width = 0, half_full = 0, partial = 0, inputs = 0, height = 0;
    if (fscanf(f, "%d %d %d %d %d %d", &curve, &width, &half_full, &partial, &inputs, &height) != 6) return 2;
    wd::Shape s;
    int rc = 9;   // a shape the circuit does not have
    if (wd::shape_make(width, half_full, partial, inputs, height, s)) rc = curve == 0 ? run<Bn254Fr>(f, s) : run<Bls381Fr>(f, s);
    fclose(f);
    return rc;
}
