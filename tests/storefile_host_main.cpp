// Stand-alone driver of csrc/storefile.hpp for tests/test_storefile_host.py: built as plain C++ with AddressSanitizer and
// UndefinedBehaviorSanitizer and run as a child process.  It follows a manifest of commands, one a line:
//   curve <0|1>
//   notes <k>            then k lines "leaf_index amount id0..id3 s0..s3" (Montgomery words): writes <out>/notes.bin, reads it
//                        back through both calls of the parser and compares
//   badnotes <path>      prints "notes <kind> <offset>"
//   treeout <E> <count>  then E lines "layer idx w0..w3" and one line "w0..w3" (the root): writes <out>/tree.bin
//   badwrite             a note whose secret's limbs equal the modulus: must be refused and leave no file
//   tree <path> <height> <capacity> <chunk>   the chunked reader; prints "tree <kind> <offset> <entries> <next_index> <read>"
#include "../zkt-plonk_amd/csrc/storefile.hpp"

#include <fstream>
#include <iostream>
#include <sstream>

using namespace zkt;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    const std::string out = argv[2];
    std::string line, cmd;
    int curve = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        if (!(ls >> cmd)) continue;
        if (cmd == "curve") {
            ls >> curve;
        } else if (cmd == "notes") {
            size_t k = 0;
            ls >> k;
            std::vector<uint64_t> li(k), am(k), id(4 * k), se(4 * k);
            for (size_t i = 0; i < k; ++i) {
                in >> li[i] >> am[i];
                for (int j = 0; j < 4; ++j) in >> id[4 * i + j];
                for (int j = 0; j < 4; ++j) in >> se[4 * i + j];
            }
            std::getline(in, line);
            const std::string path = out + "/notes.bin";
            {
                kw::File w(path.c_str());
                sf::write_notes(w, curve, li.data(), id.data(), am.data(), se.data(), k);
                if (!w.commit()) {
                    std::cout << "notes_write failed " << w.error() << "\n";
                    return 1;
                }
            }
            std::vector<uint8_t> buf;
            if (!sf::read_whole_file(path.c_str(), buf)) return 1;
            size_t n = 0;
            uint64_t off = 0;
            int kind = sf::parse_notes(buf.data(), buf.size(), curve, 0, nullptr, nullptr, nullptr, nullptr, &n, &off);
            std::vector<uint64_t> li2(n), am2(n), id2(4 * n), se2(4 * n);
            if (!kind) kind = sf::parse_notes(buf.data(), buf.size(), curve, n, li2.data(), id2.data(), am2.data(), se2.data(), &n, &off);
            const bool same = !kind && n == k && li2 == li && am2 == am && id2 == id && se2 == se;
            // one buffer too small is refused, nothing written past it
            size_t n3 = 0;
            const int small = k ? sf::parse_notes(buf.data(), buf.size(), curve, k - 1, li2.data(), id2.data(), am2.data(), se2.data(), &n3, &off) : -1;
            std::cout << "notes_roundtrip " << (same ? "ok" : "differs") << " " << n << " " << small << "\n";
        } else if (cmd == "badnotes") {
            std::string path;
            ls >> path;
            std::vector<uint8_t> buf;
            if (!sf::read_whole_file(path.c_str(), buf)) return 1;
            size_t n = 0;
            uint64_t off = 0;
            const int kind = sf::parse_notes(buf.data(), buf.size(), curve, 0, nullptr, nullptr, nullptr, nullptr, &n, &off);
            std::cout << "notes " << kind << " " << off << "\n";
        } else if (cmd == "treeout") {
            size_t E = 0;
            uint64_t count = 0;
            ls >> E >> count;
            const kw::Field& fr = kw::field(curve, false);
            const std::string path = out + "/tree.bin";
            kw::File w(path.c_str());
            sf::write_tree_head(w, E);
            uint64_t v[4];
            for (size_t i = 0; i < E; ++i) {
                uint64_t layer = 0, idx = 0;
                in >> layer >> idx >> v[0] >> v[1] >> v[2] >> v[3];
                sf::write_tree_entry(w, fr, layer, idx, v);
            }
            in >> v[0] >> v[1] >> v[2] >> v[3];
            std::getline(in, line);
            sf::write_tree_tail(w, fr, v, count);
            if (!w.commit()) {
                std::cout << "tree_write failed " << w.error() << "\n";
                return 1;
            }
            std::cout << "tree_written " << E << "\n";
        } else if (cmd == "badwrite") {
            const kw::Field& fr = kw::field(curve, false);
            uint64_t li = 1, am = 2, id[4] = {3, 0, 0, 0}, se[4];
            memcpy(se, fr.mod, 32);
            const std::string path = out + "/bad.bin";
            kw::File w(path.c_str());
            sf::write_notes(w, curve, &li, id, &am, se, 1);
            std::cout << "refused " << (w.commit() ? 0 : 1) << " " << w.error() << "\n";
        } else if (cmd == "tree") {
            std::string path;
            int height = 0;
            uint64_t capacity = 0;
            size_t chunk = 1;
            ls >> path >> height >> capacity >> chunk;
            sf::TreeFile f;
            uint64_t read = 0;
            if (f.open(path.c_str(), kw::field(curve, false), height, capacity)) {
                std::vector<uint8_t> buf(chunk * sf::TREE_ENTRY_BYTES);
                while (const size_t cnt = f.next(buf.data(), chunk)) read += cnt;
                f.finish();
            }
            std::cout << "tree " << f.kind() << " " << f.offset() << " " << f.entries() << " " << f.next_index() << " " << read << "\n";
        } else {
            return 3;
        }
    }
    return 0;
}
