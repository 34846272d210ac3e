// Stand-alone driver of the code the host and the batch verifier's kernel share -- the transcripts of
// csrc/transcript_core.hpp, the built-in host transcript on top of them (csrc/transcript.hip), compute_r0 of
// csrc/linearisation.hpp -- compiled for the host only with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_verify_core_host.py and run as a child process.  No input; prints "ok" and exits 0, or names what failed.
//   1. merlin's conformance vector and the three answers of the reference's EthereumTranscript test, through the core at a
//      stride of 1 and at a stride of 64 over an array laid out [word][lane], lane j having absorbed j scalars first; every
//      lane equals the run of its own traffic at a stride of one.
//   2. a Merlin message across two STROBE block edges: as one append_message, as scalars fed one by one, and on the core.
//   3. compute_r0 on both scalar fields, one under each inversion: no public input, one, and a root equal to xi.
#include "../zkt-plonk_amd/csrc/transcript.hip"
#include "../zkt-plonk_amd/csrc/linearisation.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace zkt;

static int failures = 0;
static void check(bool ok, const std::string& what) {
    if (ok) return;
    ++failures;
    fprintf(stderr, "FAILED: %s\n", what.c_str());
}

static std::string hex(const uint8_t* b, size_t n, bool reversed = false) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t v = b[reversed ? n - 1 - i : i];
        s += d[v >> 4];
        s += d[v & 15];
    }
    return s;
}

// `lanes` core transcripts over one array laid out [word][lane]
struct Lanes {
    uint32_t n;
    std::vector<uint64_t> words;
    std::vector<VtTr> tr;
    Lanes(uint32_t lanes, const TranscriptState& from) : n(lanes), words((size_t)VT_LANE_WORDS * lanes, 0), tr(lanes) {
        for (uint32_t j = 0; j < n; ++j) {
            tr[j].s = VtSponge{words.data() + j, words.data() + (size_t)VT_ST_WORDS * n + j,
                               words.data() + (size_t)(VT_ST_WORDS + VT_MSG_WORDS) * n + j, n};
            vt_load_state(tr[j], &from);
        }
    }
    void put(uint32_t j, const void* bytes, size_t len) {   // into lane j's message buffer, from byte 0
        for (uint32_t i = 0; i < len; ++i) vt_set_byte(tr[j].s.msg, n, i, ((const uint8_t*)bytes)[i]);
    }
    void scalar(uint32_t j, const char* label, uint64_t v) {
        uint8_t le[32] = {0};
        memcpy(le, &v, 8);
        vt_tr_scalars_begin(tr[j], label, 1);
        put(j, le, 32);
        vt_tr_scalars_item(tr[j]);
    }
    std::string challenge(uint32_t j, const char* label, uint32_t bits, bool reversed) {
        uint32_t w[8];
        vt_tr_challenge(tr[j], label, bits, w);
        return hex((const uint8_t*)w, 32, reversed);
    }
    TranscriptState state(uint32_t j) {
        TranscriptState st;
        vt_store_state(tr[j], &st);
        return st;
    }
};

// lane j absorbs j scalars, then every lane the traffic of the known answers; step by step across the lanes, so that a
// lane writing outside its own words would spoil a neighbour that is still at work
static std::vector<std::string> known_answer_traffic(Lanes& L, uint32_t first_lane_extra) {
    std::vector<std::string> out(L.n);
    for (uint32_t e = 0; e < first_lane_extra + L.n - 1; ++e)
        for (uint32_t j = 0; j < L.n; ++j)
            if (e < first_lane_extra + j) L.scalar(j, "extra", 0x0123456789abcdefULL * (e + 1));
    if (L.tr[0].kind == 0) {
        for (uint32_t j = 0; j < L.n; ++j) {
            vt_merlin_header(L.tr[j], "some label", 9);
            vt_begin_op(L.tr[j], VT_FLAG_A);
            L.put(j, "some data", 9);
            vt_absorb_msg(L.tr[j], 9);
        }
        for (uint32_t j = 0; j < L.n; ++j) out[j] = L.challenge(j, "challenge", 264, false);   // 264 bits: 32 bytes of prf
        return out;
    }
    // gadgets/src/transcript.rs:101-127: a u64, a scalar and a commitment, a challenge behind each
    for (uint32_t j = 0; j < L.n; ++j) {
        const uint64_t one = 1;
        L.put(j, &one, 8);
        vt_eth_append(L.tr[j], 0, 8);
    }
    for (uint32_t j = 0; j < L.n; ++j) out[j] = L.challenge(j, "a", 254, true);
    for (uint32_t j = 0; j < L.n; ++j) L.scalar(j, "b", 2);
    for (uint32_t j = 0; j < L.n; ++j) out[j] += " " + L.challenge(j, "b", 254, true);
    for (uint32_t j = 0; j < L.n; ++j) {
        uint8_t xy[65] = {0};
        xy[0] = 3;
        xy[32] = 4;
        L.put(j, xy, 65);
        vt_tr_commit_msg(L.tr[j], "c", 32);
    }
    for (uint32_t j = 0; j < L.n; ++j) out[j] += " " + L.challenge(j, "c", 254, true);
    return out;
}

static void known_answers() {
    const char* want[2] = {"d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615",
                           "0f9d11cec4f06b0d18060cde3db4196495ddfbb096108951446fc8a1d45f4b59 "
                           "0f4dccb919a5dba2dd010a562ba45b4551291f5e565706536e78b24ac8b5c64d "
                           "1b5bf46adfcd1dd4f9ac7166586cf83f261192bc4b83fdda30ddee22f9054c1f"};
    for (int kind = 0; kind < 2; ++kind) {
        const std::string who = kind == 0 ? "merlin" : "ethereum";
        BuiltinTranscript seeded(kind, kind == 0 ? "test protocol" : "test");
        TranscriptState from;
        check(seeded.export_state(from), who + ": export_state");
        Lanes wide(64, from);
        const std::vector<std::string> got = known_answer_traffic(wide, 0);
        check(got[0] == want[kind], who + ": the known answers at a stride of 64, lane 0: " + got[0]);
        for (uint32_t j = 0; j < 64; ++j) {
            Lanes one(1, from);
            const std::string alone = known_answer_traffic(one, j)[0];
            if (j == 0) check(alone == want[kind], who + ": the known answers at a stride of 1: " + alone);
            check(got[j] == alone, who + ": lane " + std::to_string(j) + " against its own run at a stride of one");
            const TranscriptState a = wide.state(j), b = one.state(0);
            check(memcmp(&a, &b, sizeof a) == 0, who + ": lane " + std::to_string(j) + " is left in another state");
        }
    }
}

// 13 scalars = 416 bytes in ONE message: from position p the message covers the block edges at 166 and 332
static void long_message() {
    uint8_t msg[416];
    for (size_t i = 0; i < sizeof msg; ++i) msg[i] = (uint8_t)(i * 37 + 11);
    BuiltinTranscript whole(0, "ZKT Plonk"), items(0, "ZKT Plonk"), seeded(0, "ZKT Plonk");
    check(whole.append_message("pi", msg, sizeof msg), "append_message");
    items.append_scalars("pi", msg, 13, 32, false);
    TranscriptState from;
    seeded.export_state(from);
    Lanes core(1, from);
    vt_tr_scalars_begin(core.tr[0], "pi", 13);
    for (int k = 0; k < 13; ++k) {
        core.put(0, msg + 32 * k, 32);
        vt_tr_scalars_item(core.tr[0]);
    }
    TranscriptState a, b;
    whole.export_state(a);
    items.export_state(b);
    const TranscriptState c = core.state(0);
    check(memcmp(&a, &b, sizeof a) == 0, "a 416-byte message: one append_message against 13 scalars under one label");
    check(memcmp(&a, &c, sizeof a) == 0, "a 416-byte message: the host class against the core fed item by item");
    uint8_t x[48], y[48];
    check(whole.challenge_bytes("after", x, sizeof x) && items.challenge_bytes("after", y, sizeof y), "challenge_bytes");
    check(memcmp(x, y, sizeof x) == 0, "the challenge behind the 416-byte message");
    // a state is refused as a whole: nothing changes
    TranscriptState bad = a;
    bad.pos = VT_RATE;
    check(!items.import_state(bad), "a position outside the rate is refused");
    bad = a;
    bad.kind = 1;
    check(!items.import_state(bad), "the other kind's state is refused");
    items.export_state(b);
    whole.export_state(a);
    check(memcmp(&a, &b, sizeof a) == 0, "a refused state changes nothing");
    BuiltinTranscript eth(1, "");
    check(!eth.append_message("x", msg, 4) && !eth.challenge_bytes("x", x, 4), "merlin's own calls on the other kind");
}

// compute_r0 as one function per field and inversion (at most two public inputs)
template <class R, Fe<R> (*INV)(const Fe<R>&)>
__attribute__((noinline)) static bool r0_of(const Challenges<R>& ch, const XiPoint<R>& at, const Fe<R>* ev, const Fe<R>* roots,
                                            const Fe<R>* vals, uint64_t k, Fe<R>* out) {
    Fe<R> before[2];
    return compute_r0<R, INV>(ch, at, ev, roots, vals, k, before, out);
}

template <class R, Fe<R> (*INV)(const Fe<R>&)>
static void r0_cases(const std::string& who) {
    typedef Fe<R> F;
    auto fe = [](uint64_t v) { return fe_from_u64<R>(v * 0x9e3779b97f4a7c15ULL + 12345); };
    const Challenges<R> ch{fe(1), fe(2), fe(3), fe(4), fe(5), fe(6), fe_zero<R>()};
    XiPoint<R> at;
    check(xi_point<R, INV>(ch, 16, at), who + ": xi_point");
    Challenges<R> one = ch;
    one.xi = fe_one<R>();
    XiPoint<R> unused;
    check(!xi_point<R, INV>(one, 16, unused), who + ": xi = 1 has no L_1");
    F ev[EV_COUNT];
    for (int k = 0; k < EV_COUNT; ++k) ev[k] = fe(20 + k);
    const F root = fe(40), val = fe(41), val_on_xi = fe(42);
    F none, single, two;
    check(!r0_of<R, INV>(ch, at, ev, nullptr, nullptr, 0, &none), who + ": k = 0 has no denominator");
    check(!r0_of<R, INV>(ch, at, ev, &root, &val, 1, &single), who + ": k = 1, a root off xi");
    // L(xi) = zh root / (n (xi - root)), by the other formula: one inversion of its own
    const F lag = fe_mul<R>(fe_mul<R>(at.zh, root), INV(fe_mul<R>(at.nn, fe_sub<R>(ch.xi, root))));
    check(fe_eq<R>(single, fe_sub<R>(none, fe_mul<R>(lag, val))), who + ": k = 1 is k = 0 less L(xi) val");
    const F roots[2] = {ch.xi, root}, vals[2] = {val_on_xi, val};
    check(r0_of<R, INV>(ch, at, ev, roots, vals, 2, &two), who + ": a root equal to xi is reported");
    check(fe_eq<R>(two, fe_sub<R>(single, val_on_xi)), who + ": a root equal to xi contributes -val");
    const F roots_r[2] = {root, ch.xi}, vals_r[2] = {val, val_on_xi};
    check(r0_of<R, INV>(ch, at, ev, roots_r, vals_r, 2, &two) && fe_eq<R>(two, fe_sub<R>(single, val_on_xi)),
          who + ": ... wherever it stands");
    check(r0_of<R, INV>(ch, at, ev, &ch.xi, &val_on_xi, 1, &two) && fe_eq<R>(two, fe_sub<R>(none, val_on_xi)),
          who + ": k = 1 with its root on xi");
}

int main() {
    known_answers();
    long_message();
    r0_cases<Bn254Fr, fe_inv_host<Bn254Fr>>("bn254, the host's inversion");
    r0_cases<Bls381Fr, fe_inv_call<Bls381Fr>>("bls12_381, the kernels' inversion");
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
