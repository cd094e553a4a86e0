// The option table (rawalign_amd/csrc/rawdtw_options.h) held to what the hand-written setter did before it: a stand-alone program, no HIP,
// no library.  tests/test_options_cpu.py writes the records of tests/option_cases.py to a file, one a line:
//   default NAME VALUE             the field of a fresh record
//   case NAME VALUE STATUS STORED [MESSAGE]   set(NAME, VALUE) on a fresh record: its status, get(NAME) after it, the refusal's text
//   refused NAME STATUS MESSAGE    a name no setter takes (the computed rows, a name nobody knows)
// and this program checks every line, that no name occurs twice and that every row was asked about.  `options --names` prints the rows'
// names, the computed ones marked, for the test that reads include/rawdtw.h.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <set>
#include <sstream>

#include "rawdtw_options.h"

using namespace rawdtw;

static int bad = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { bad++; fprintf(stderr, "line %d: ", line_no); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--names")) {
        for (const opt::Row &r : opt::kRows) printf("%s%s\n", r.name, (r.flags & opt::kReadOnly) ? " read-only" : "");
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: options CASES | --names\n"); return 2; }
    int line_no = 0;
    std::set<std::string> names, with_default, with_case, refused;
    for (const opt::Row &r : opt::kRows) CHECK(names.insert(r.name).second, "row %s occurs twice", r.name);
    CHECK(names.size() == opt::kNumRows && opt::kNumSettable < opt::kNumRows, "the rows' count");
    for (size_t i = 0; i < opt::kNumRows; i++) // the computed rows are the last ones, and only they are read-only
        CHECK(((opt::kRows[i].flags & opt::kReadOnly) != 0) == (i >= opt::kNumSettable) && (opt::kRows[i].store != nullptr) == (i < opt::kNumSettable) &&
              (opt::kRows[i].load != nullptr) == (i < opt::kNumSettable), "row %s: read-only and its place", opt::kRows[i].name);

    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    long cases = 0;
    while (std::getline(in, line)) {
        line_no++;
        std::istringstream ls(line);
        std::string kind, name, message;
        ls >> kind >> name;
        Options o; // (a fresh record for every line)
        int64_t got = 0;
        if (kind == "default") {
            int64_t want = 0;
            ls >> want;
            CHECK(!ls.fail() && opt::get(o, name.c_str(), &got) == RAWDTW_OK && got == want, "default of %s: %" PRId64 ", recorded %" PRId64, name.c_str(), got, want);
            with_default.insert(name);
        } else if (kind == "case") {
            int64_t value = 0, stored = 0;
            int status = 0;
            ls >> value >> status >> stored;
            CHECK(!ls.fail(), "unreadable case");
            std::getline(ls >> std::ws, message);
            std::string err;
            const int st = opt::set(o, name.c_str(), value, err);
            CHECK(st == status, "%s = %" PRId64 ": status %d, recorded %d", name.c_str(), value, st, status);
            CHECK(opt::get(o, name.c_str(), &got) == RAWDTW_OK && got == stored, "%s = %" PRId64 ": stored %" PRId64 ", recorded %" PRId64, name.c_str(), value, got, stored);
            CHECK(err == message && (st == RAWDTW_OK) == err.empty(), "%s = %" PRId64 ": said \"%s\", recorded \"%s\"", name.c_str(), value, err.c_str(), message.c_str());
            CHECK(o.tile_lds_set == (name == "tile_lds_floats"), "%s: tile_lds_set", name.c_str());
            with_case.insert(name);
            cases++;
        } else if (kind == "refused") {
            int status = 0;
            ls >> status;
            std::getline(ls >> std::ws, message);
            std::string err;
            CHECK(opt::set(o, name.c_str(), 1, err) == status && status != RAWDTW_OK && err == message, "set of %s: said \"%s\", recorded \"%s\"", name.c_str(), err.c_str(), message.c_str());
            CHECK(opt::get(o, name.c_str(), &got) == RAWDTW_ERR_INVALID, "get of %s on a record alone", name.c_str());
            refused.insert(name);
        } else CHECK(false, "unknown line \"%s\"", line.c_str());
    }
    line_no = 0;
    // every row was asked about: a settable one has a default and cases, a computed one is among the refused; and nothing else was
    size_t settable = 0;
    for (const opt::Row &r : opt::kRows) {
        const bool ro = (r.flags & opt::kReadOnly) != 0;
        settable += !ro;
        CHECK(ro ? refused.count(r.name) == 1 : with_default.count(r.name) == 1 && with_case.count(r.name) == 1, "row %s has no record", r.name);
    }
    CHECK(with_default.size() == settable && with_case.size() == settable && refused.size() == opt::kNumRows - settable + 1, "records of names that are no rows");
    if (bad) { fprintf(stderr, "%d failures\n", bad); return 1; }
    printf("ok %zu %ld\n", opt::kNumRows, cases);
    return 0;
}
