// McIlroy's adversary ("A killer adversary for quicksort", 1999) against this machine's std::sort with the comparator of rmap.cpp:512
// (score descending): the comparator decides values lazily -- an element is "gas" until a comparison of two gas elements forces one to
// become solid, and it is always the one that is not the current pivot candidate, so every pivot turns out to be among the smallest keys of
// its range, the partitions peel a few elements each and the depth budget runs out.  The values it assigned are then frozen and printed as
// scores, one a line: an input that drives std::sort -- and whatever claims to restate it -- into the heap phase.
//   usage: sort_adversary N
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static std::vector<int> val; // the key of an element: sorted ascending by it (score = -key); gas while undecided
static int gas, nsolid, candidate;

static bool before(int x, int y)
{
    if (val[x] == gas && val[y] == gas) {
        if (x == candidate) val[x] = nsolid++;
        else val[y] = nsolid++;
    }
    if (val[x] == gas) candidate = x;
    else if (val[y] == gas) candidate = y;
    return val[x] < val[y];
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 100;
    if (n < 1 || n > (1 << 20)) return 2;
    gas = n; nsolid = 0; candidate = 0;
    val.assign((size_t)n, gas);
    std::vector<int> ptr((size_t)n);
    for (int i = 0; i < n; i++) ptr[(size_t)i] = i;
    std::sort(ptr.begin(), ptr.end(), before);
    for (int i = 0; i < n; i++) printf("%d\n", 2 * n - val[(size_t)i]); // (a positive score that falls as the key rises; what stayed gas ties)
    return 0;
}
