// Stand-alone driver of the key-file writers (csrc/keyfile_write.hpp, which includes nothing of HIP): writes the --ck, --pk
// and --vk files of a case, parses them back with a reader of its own and prints what it found.  Compiled as plain C++ with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_keyfile_write_host.py and run as a child process.
//
// Input file (text, 64-bit words in decimal, Montgomery limbs):  curve count n n_pi / count lines of one point (8 or 12
// words) / ten lines "len" then 4 len words / n_pi lines of 4 words / ten lines of one point and its infinity flag.
// Files: <outdir>/ck.bin pk.bin vk.bin; a fourth write, of a coefficient equal to the modulus, must be refused.
// Output:  "ck count gamma_count max_degree" and per point "x y infinity" (hex); "pk" and per polynomial "label len" then the
// values; "vk n n_pi", the roots, the ten points; "refused <0|1> <message>".
#include "../zkt-plonk_amd/csrc/keyfile_write.hpp"

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

using namespace zkt;

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Reader {
    const std::vector<uint8_t>& b;
    size_t pos = 0;
    const uint8_t* take(size_t k) {
        if (k > b.size() - pos) {
            std::cerr << "parse: file too short\n";
            exit(3);
        }
        const uint8_t* p = b.data() + pos;
        pos += k;
        return p;
    }
    uint64_t u64() {
        const uint8_t* p = take(8);
        uint64_t v = 0;
        for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
        return v;
    }
    uint8_t u8() { return *take(1); }
    std::string hex(size_t nb, unsigned strip_top_bits = 0) {   // a little-endian value as big-endian hex
        const uint8_t* p = take(nb);
        static const char* d = "0123456789abcdef";
        std::string s;
        for (size_t i = nb; i-- > 0;) {
            uint8_t v = p[i];
            if (i == nb - 1 && strip_top_bits) v &= (uint8_t)(0xFF >> strip_top_bits);
            s += d[v >> 4];
            s += d[v & 15];
        }
        return s;
    }
    void point(size_t nb) {
        const std::string x = hex(nb);
        const uint8_t flags = b.at(pos + nb - 1);
        const std::string y = hex(nb, 2);
        std::cout << x << " " << y << " " << ((flags & 0x40) ? 1 : 0) << "\n";
    }
    void end() {
        if (pos != b.size()) {
            std::cerr << "parse: trailing bytes\n";
            exit(3);
        }
    }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    const std::string dir = argv[2];
    int curve = 0;
    size_t count = 0, n = 0, n_pi = 0;
    in >> curve >> count >> n >> n_pi;
    const size_t words = curve == 0 ? 8 : 12, nb = words * 4;
    std::vector<uint64_t> powers(count * words);
    for (auto& v : powers) in >> v;
    std::vector<std::vector<uint64_t>> polys(10);
    const uint64_t* ptrs[10];
    size_t lens[10];
    for (int k = 0; k < 10; ++k) {
        in >> lens[k];
        polys[k].resize(4 * lens[k]);   // (a polynomial of length 0 has no storage at all)
        for (auto& v : polys[k]) in >> v;
        ptrs[k] = polys[k].data();
    }
    std::vector<uint64_t> roots(4 * n_pi), commits(10 * words);
    for (auto& v : roots) in >> v;
    int inf[10];
    for (int k = 0; k < 10; ++k) {
        for (size_t i = 0; i < words; ++i) in >> commits[k * words + i];
        in >> inf[k];
    }
    if (!in) return 2;

    {
        kw::File w((dir + "/ck.bin").c_str());
        kw::write_committer_key(w, curve, powers.data(), count);
        if (!w.commit()) return std::cerr << w.error() << "\n", 1;
    }
    {
        kw::File w((dir + "/pk.bin").c_str());
        kw::write_prover_key(w, curve, ptrs, lens);
        if (!w.commit()) return std::cerr << w.error() << "\n", 1;
    }
    {
        kw::File w((dir + "/vk.bin").c_str());
        kw::write_verifier_key(w, curve, n, roots.data(), n_pi, commits.data(), inf);
        if (!w.commit()) return std::cerr << w.error() << "\n", 1;
    }

    {
        const std::vector<uint8_t> b = slurp(dir + "/ck.bin");
        Reader r{b};
        const uint64_t c = r.u64();
        std::vector<size_t> at;
        for (uint64_t i = 0; i < c; ++i) {
            at.push_back(r.pos);
            r.take(2 * nb);
        }
        const uint64_t gamma = r.u64();
        const int none = r.u8() + r.u8() + r.u8();
        const uint64_t max_degree = r.u64();
        r.end();
        if (none != 0) return std::cerr << "ck: an Option is not None\n", 3;
        std::cout << "ck " << c << " " << gamma << " " << max_degree << "\n";
        for (size_t p : at) {
            r.pos = p;
            r.point(nb);
        }
    }
    {
        const std::vector<uint8_t> b = slurp(dir + "/pk.bin");
        Reader r{b};
        std::cout << "pk\n";
        for (int k = 0; k < 10; ++k) {
            const uint64_t ll = r.u64();
            const uint8_t* l = r.take(ll);
            const std::string label(l, l + ll);
            const uint64_t len = r.u64();
            std::cout << label << " " << len << "\n";
            for (uint64_t i = 0; i < len; ++i) std::cout << r.hex(32) << "\n";
            if (r.u8() != 0 || r.u8() != 0) return std::cerr << "pk: a bound is not None\n", 3;
        }
        r.end();
    }
    {
        const std::vector<uint8_t> b = slurp(dir + "/vk.bin");
        Reader r{b};
        const uint64_t vn = r.u64(), k = r.u64();
        std::cout << "vk " << vn << " " << k << "\n";
        for (uint64_t i = 0; i < k; ++i) std::cout << r.hex(32) << "\n";
        for (int j = 0; j < 10; ++j) r.point(nb);
        r.end();
    }
    {   // a coefficient equal to the modulus: refused, and neither bad.bin nor its temporary file stays
        const kw::Field& fr = kw::field(curve, false);
        uint64_t p[4];
        memcpy(p, fr.mod, 32);
        const uint64_t* one[10] = {p};
        size_t l[10] = {1};
        kw::File w((dir + "/bad.bin").c_str());
        kw::write_prover_key(w, curve, one, l);
        const bool done = w.commit();
        std::cout << "refused " << (done ? 0 : 1) << " " << w.error() << "\n";
    }
    return 0;
}
