// Host driver of fx_mul3_inl (csrc/fx.hpp) for tests/test_fx_mul3_host.py: reads records "field l0 .. l(6L-1)" (field:
// 0 BN254 Fr, 1 BLS12-381 Fr, 2 BN254 Fq, 3 BLS12-381 Fq; the limbs of a b c d e f in order) from standard input and
// prints the L limbs of (a b + c d + e f) / R' per record.  Host code only: nothing here touches a device.
#include <cstdio>
#include <cstdint>

#include "../zkt-plonk_amd/csrc/fx.hpp"

using namespace zkt;

template <class P>
static bool one_record() {
    constexpr int L = FxP<P>::L;
    Fx<P> v[6];
    for (int k = 0; k < 6; ++k)
        for (int i = 0; i < L; ++i) {
            unsigned long long x;
            if (scanf("%llu", &x) != 1 || x > 0xffffffffull) return false;
            v[k].l[i] = (uint32_t)x;
        }
    const Fx<P> r = fx_mul3_inl<P>(v[0], v[1], v[2], v[3], v[4], v[5]);
    for (int i = 0; i < L; ++i) printf(i + 1 < L ? "%u " : "%u\n", r.l[i]);
    return true;
}

int main() {
    int field;
    while (scanf("%d", &field) == 1) {
        bool ok = false;
        switch (field) {
            case 0: ok = one_record<Bn254Fr>(); break;
            case 1: ok = one_record<Bls381Fr>(); break;
            case 2: ok = one_record<Bn254Fq>(); break;
            case 3: ok = one_record<Bls381Fq>(); break;
        }
        if (!ok) return 2;
    }
    return 0;
}
