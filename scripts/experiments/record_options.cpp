// record_options.cpp -- what rawdtw_set_option does with every settable option at a list of probe values, written as the data of
// tests/option_cases.py.  Run at commit 97069d5 ("Test the index build past its thresholds"), the parent of the change that put the
// options into one table (rawdtw_options.h): the recorded behaviour is that commit's hand-written setter's, not the table's.
//
// A default-constructed context record needs no HIP call, so this runs without a GPU:
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Irawalign_amd/csrc scripts/experiments/record_options.cpp
//       rawalign_amd/librawdtw.so -Wl,-rpath,$PWD/rawalign_amd -o record_options && ./record_options > tests/option_cases.py
// Per (name, value), on a fresh record: the status, the value the field then holds, and rawdtw_last_error where the setter refused.
// The values are the common list below plus, for each option, each of its bounds minus one, exact and plus one.
#include <cinttypes>
#include <climits>
#include <cstdio>
#include <set>
#include <vector>

#include "rawdtw_capi.h"

namespace {

const int64_t kCommon[] = {INT64_MIN, -1, 0, 1, 2, 255, 256, 511, 512, 1023, 1024, 4096, 4097, 40000, 40001, 65535, 65536, 1 << 20, (1 << 20) + 1,
                           (1 << 24) + 1, (1 << 30) + 1, INT32_MAX, 1ll << 31, UINT32_MAX, 1ll << 32, INT64_MAX};

struct Opt {
    const char *name;
    int64_t (*field)(const rawdtw_ctx &);
    std::vector<int64_t> bounds; // read off the setter's source at that commit
};
#define OPT(name, ...) {#name, [](const rawdtw_ctx &c) { return (int64_t)c.name; }, {__VA_ARGS__}}
const Opt kOpts[] = {
    OPT(serial_launches, 0, 1), OPT(tile_lds_floats, 1024, 40000), OPT(tile_max_jobs, 64, 65535), OPT(plan_threads, 0, 64),
    OPT(debug_skip_kinds, 0, UINT32_MAX), OPT(pass_pool, -1, 1 << 24), OPT(wide_at_create, 0, 1), OPT(wide_order, 0, 2), OPT(wide_beside, 0, 1),
    OPT(wide_blocks, 1, 65535), OPT(debug_skip_tail, 0, UINT32_MAX), OPT(sort_n, 0, 255), OPT(sort_r1_n, 0, 255), OPT(sort_r3, 0, 1),
    OPT(sorted_tile_jobs, 16, 1024), OPT(device_plan, 0, 1), OPT(device_plan_min_jobs, 0, INT64_MAX), OPT(stream_blocks_per_cu, 0, 16),
    OPT(stream_threads, 256, 512), OPT(stream_debug, 0, UINT32_MAX), OPT(resident_arrays, 0, 1), OPT(time_plan, 0, 1), OPT(merge_small, 0, 1),
    OPT(fold_mode, 0, 4), OPT(fold_long_parts, 1, 1 << 30), OPT(tile_threads, 256, 512, 1024), OPT(tile_max_spans, 8, 4096), OPT(full_wg, 0, 1),
    OPT(grp16, 0, 1), OPT(grp8, 0, 1), OPT(micro_max_n, 0, 4, 8), OPT(lane_hi_max_n, 8, 200), OPT(lane_hi, 0, 1), OPT(lane_max_n, 8, 73),
    OPT(stream_tile_radius, 1, 3), OPT(chain_long_seeds, 0, 1 << 20), OPT(chain_max_chains, 0, 4096), OPT(chain_decline_reads, 0, 1),
    OPT(seed_minimizer, 0, 1), OPT(device_round_end, 0, 1), OPT(resident_chains, 0, 1 << 20), OPT(signal_events_cap, 0, INT64_MAX),
    OPT(signal_cigar, 0, 1), OPT(tb_workspace_mb, 0, 1 << 30), OPT(lane_max_radius, 0, 3),
};
const char *const kReadOnly[] = {"tb_sub_batches", "round_end_kernel_us", "round_keep_kernel_us"};

void py_string(const char *s)
{
    putchar('\'');
    for (; *s; s++) { if (*s == '\'' || *s == '\\') putchar('\\'); putchar(*s); }
    putchar('\'');
}

// does rawdtw_plan_dry_run take the name?  (an empty job list: the options are read before anything else)
bool dry_run_takes(const char *name, char *message, uint32_t cap)
{
    const int64_t v = 1;
    return rawdtw_plan_dry_run(0, 0, nullptr, 0, 1, &name, &v, 1, nullptr, nullptr, message, cap) == RAWDTW_OK;
}

} // namespace

int main()
{
    printf("\"\"\"What rawdtw_set_option did with every settable option before the options were put into one table (rawalign_amd/csrc/rawdtw_options.h):\n"
           "the output of scripts/experiments/record_options.cpp at commit 97069d5, on a default-constructed context record, without a GPU.\n"
           "tests/test_options_cpu.py holds the table to it, tests/test_options_gpu.py a live context.\n\n"
           "DEFAULTS  name -> the field of a fresh record\n"
           "CASES     name -> [(value, status, the field after rawdtw_set_option(name, value) on a fresh record, rawdtw_last_error or None)]\n"
           "PLANNER   the names rawdtw_plan_dry_run took (besides its own \"verify\")\n"
           "READ_ONLY the names rawdtw_get_option answered and rawdtw_set_option refused; REFUSED: name -> (status, message) of that refusal, and of\n"
           "          a name nobody knows\"\"\"\n\n");
    printf("DEFAULTS = {\n");
    for (const Opt &o : kOpts) { rawdtw_ctx c; printf("    '%s': %" PRId64 ",\n", o.name, o.field(c)); }
    printf("}\n\nCASES = {\n");
    for (const Opt &o : kOpts) {
        std::set<int64_t> seen;
        std::vector<int64_t> values(std::begin(kCommon), std::end(kCommon));
        for (int64_t b : o.bounds) {
            if (b > INT64_MIN) values.push_back(b - 1);
            values.push_back(b);
            if (b < INT64_MAX) values.push_back(b + 1);
        }
        printf("    '%s': [\n", o.name);
        for (int64_t v : values) {
            if (!seen.insert(v).second) continue;
            rawdtw_ctx c;
            const int st = rawdtw_set_option(&c, o.name, v);
            printf("        (%" PRId64 ", %d, %" PRId64 ", ", v, st, o.field(c));
            if (st == RAWDTW_OK) printf("None"); else py_string(rawdtw_last_error(&c));
            printf("),\n");
        }
        printf("    ],\n");
    }
    printf("}\n\nPLANNER = [");
    char msg[256];
    for (const Opt &o : kOpts) if (dry_run_takes(o.name, msg, sizeof msg)) printf("'%s', ", o.name);
    printf("]\n\nREAD_ONLY = [");
    for (const char *n : kReadOnly) printf("'%s', ", n);
    printf("]\n\nREFUSED = {\n");
    for (const char *n : {kReadOnly[0], kReadOnly[1], kReadOnly[2], "no_such_option"}) {
        rawdtw_ctx c;
        const int st = rawdtw_set_option(&c, n, 1);
        printf("    '%s': (%d, ", n, st); py_string(rawdtw_last_error(&c)); printf("),\n");
    }
    printf("}\n");
    return 0;
}
