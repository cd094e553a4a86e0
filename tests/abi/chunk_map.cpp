// The chunk map of k_runs (rawalign_amd/csrc/rawdtw_chunks.h) as a plain C++ program: for every n3 <= 64 and
// n3 <= n_hi <= n_jobs <= 512 the chunks' ranges tile [0, n_jobs) exactly once and in order, none crosses n3 or n_hi, the quad
// chunks are exactly the first ceil(n3 / 16), and the count is ceil(n3/16) + ceil((n_hi - n3)/64) + ceil((n_jobs - n_hi)/64).
// With n_hi = n_jobs (no boundary of the radius-1 run's own) the lane chunks are cut every 64 records from n3 on.  Prints "ok <cases>"; the first failure otherwise.
#include <cstdio>

#include "rawdtw_chunks.h"

using namespace rawdtw;

static unsigned ceil_div(unsigned a, unsigned b) { return a / b + (a % b ? 1u : 0u); }

static int bad(const char *what, unsigned n3, unsigned n_hi, unsigned n_jobs, unsigned c)
{
    printf("FAIL %s: n3 %u n_hi %u n_jobs %u chunk %u\n", what, n3, n_hi, n_jobs, c);
    return 1;
}

int main()
{
    unsigned long long cases = 0;
    for (unsigned n_jobs = 0; n_jobs <= 512; n_jobs++)
        for (unsigned n_hi = 0; n_hi <= n_jobs; n_hi++)
            for (unsigned n3 = 0; n3 <= 64 && n3 <= n_hi; n3++) {
                const unsigned want_q = ceil_div(n3, 16), want = want_q + ceil_div(n_hi - n3, 64) + ceil_div(n_jobs - n_hi, 64);
                const unsigned n = chunk_map_count(n3, n_hi, n_jobs);
                if (n != want) return bad("count", n3, n_hi, n_jobs, n);
                if (chunk_map_quads(n3) != want_q) return bad("quad count", n3, n_hi, n_jobs, 0);
                unsigned at = 0; // each range starts where the one before ended, none is empty, the last ends at n_jobs: every record once
                for (unsigned c = 0; c < n; c++) {
                    const ChunkRange r = chunk_map_range(n3, n_hi, n_jobs, c);
                    if (r.first != at || r.end <= r.first || r.end > n_jobs) return bad("range out of order, empty or beyond the pass", n3, n_hi, n_jobs, c);
                    if (r.quad != (c < want_q)) return bad("quad flag", n3, n_hi, n_jobs, c);
                    if (r.end - r.first > (r.quad ? 16u : 64u)) return bad("chunk too long", n3, n_hi, n_jobs, c);
                    if (r.quad && r.end > n3) return bad("a quad chunk beyond n3", n3, n_hi, n_jobs, c);
                    if ((r.first < n3 && r.end > n3) || (r.first < n_hi && r.end > n_hi)) return bad("a chunk crosses a class boundary", n3, n_hi, n_jobs, c);
                    at = r.end;
                }
                if (at != n_jobs) return bad("records left over", n3, n_hi, n_jobs, n);
                if (n_hi == n_jobs) { // the flat map: the lane chunks cut every 64 records from n3 on
                    for (unsigned c = want_q; c < n; c++) {
                        const ChunkRange r = chunk_map_range(n3, n_hi, n_jobs, c);
                        const unsigned first = n3 + (c - want_q) * 64, end = first + 64 < n_jobs ? first + 64 : n_jobs;
                        if (r.first != first || r.end != end) return bad("flat range", n3, n_hi, n_jobs, c);
                    }
                }
                cases++;
            }
    printf("ok %llu\n", cases);
    return 0;
}
