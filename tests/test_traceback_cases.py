"""The case lists of tests/traceback_cases.py have the properties they are there for -- shown on the oracle's paths alone, no
device -- and the Python model of the traceback driver's split cuts them as the GPU tests rely on."""
import numpy as np

from tests import traceback_cases as tc


def _walk_len(want, ex):
    """path elements the walk kernel produces: the oracle's length before exclude_last's pop"""
    return len(want[1]) + int(ex)


def _longest_run(x):
    """longest run of zeros in x"""
    best = run = 0
    for z in (np.asarray(x) == 0):
        run = run + 1 if z else 0
        best = max(best, run)
    return best


def test_model_restates_the_direction_buffer_sizes():
    assert [tc.full_rpl(n) for n in (1, 64, 65, 128, 129, 256, 257, 9000)] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert tc.dir_bytes_for(8192, 8192) == 16_908_288           # the benchmark's traceback_8192 job
    assert tc.dir_bytes_for(3000, 3000) == 6 * 383 * 1024        # 2.3 MB: six strips of 383 blocks
    assert tc.dir_bytes_for(1, 1) == 4 * 1024 and tc.dir_bytes_for(300, 8192) == tc.dir_bytes_for(8192, 300)
    # a job over the budget goes alone; one that fits exactly joins
    b = tc.dir_bytes_for(64, 64) + 256
    assert tc.split([(64, 64)] * 5, 2 * b) == [(0, 2), (2, 2), (4, 1)]
    assert tc.split([(64, 64)] * 3, 1) == [(0, 1), (1, 1), (2, 1)]
    assert tc.split([(64, 64), (3000, 3000), (64, 64)], 3 * b) == [(0, 1), (1, 1), (2, 1)]
    assert tc.split([], 1) == []


def test_pipe_splits_into_many_sub_batches_with_the_large_jobs_alone():
    shapes = tc.shapes_of(tc.pipe_cases())
    assert len(shapes) == 123 and sum(n * m for n, m in shapes) > 35_000_000
    subs = tc.split(shapes, tc.MIB)
    print("PIPE at 1 MiB:", len(subs), "sub-batches of", [c for _, c in subs])
    assert len(subs) >= 6
    for k in tc.PIPE_LARGE:
        assert (k, 1) in subs, k
    assert sum(c for _, c in subs) == len(shapes) and all(c >= 1 for _, c in subs)
    assert max(c for _, c in subs) >= 8                        # (and sub-batches of many jobs: order[] within one matters)
    assert tc.split(shapes, tc.DEFAULT_BUDGET) == [(0, len(shapes))]
    assert [ex for _, _, _, ex in tc.pipe_cases()][:7] == [1, 0, 0, 1, 0, 0, 1]


def test_big_at_16_mib_puts_the_8192_square_alone():
    shapes = tc.shapes_of(tc.big_cases())
    assert tc.dir_bytes_for(*shapes[0]) > 16 * tc.MIB
    assert tc.split(shapes, 16 * tc.MIB) == [(0, 1), (1, 3)]
    assert tc.split(shapes, tc.DEFAULT_BUDGET) == [(0, 4)]


def test_edge_has_the_path_lengths_runs_and_classes(oracle):
    cases, want = tc.edge_cases(), tc.oracle_paths(oracle, "edge")
    assert [ex for _, _, _, ex in cases][:4] == [0, 1, 0, 1]
    # path lengths as the walk produces them: a full last flush, one element in the last flush, 63 in it
    residues = {_walk_len(w, c[3]) % 64 for c, w in zip(cases, want)}
    assert {0, 1, 63} <= residues, sorted(residues)
    # ... on pure diagonals too (length n), not only on one-row jobs
    diag = [(c, w) for c, w in zip(cases, want) if len(c[0]) == len(c[1]) and np.array_equal(c[0], c[1])]
    assert sorted(len(c[0]) for c, _ in diag) == sorted(tc.EDGE_IDENTICAL)
    for c, w in diag:
        assert _walk_len(w, c[3]) == len(c[0]) and w[0] == 0
    assert {len(c[0]) % 64 for c, _ in diag} == {0, 1, 63}
    # long runs along both borders, in jobs that are not one row or one column (there every step is a border step)
    two_d = [w for c, w in zip(cases, want) if min(len(c[0]), len(c[1])) > 2]
    assert max(_longest_run(w[2]) for w in two_d) >= 128     # j == 0
    assert max(_longest_run(w[1]) for w in two_d) >= 128     # i == 0
    assert max(_longest_run(w[2]) for w in two_d) >= tc.BORDER_RUN and max(_longest_run(w[1]) for w in two_d) >= tc.BORDER_RUN
    # every rows-per-lane class in both orientations, and its upper boundary as the shorter side
    shapes = tc.shapes_of(cases)
    for rpl in (1, 2, 4, 8):
        assert any(n > m and tc.full_rpl(m) == rpl for n, m in shapes), rpl
        assert any(n < m and tc.full_rpl(n) == rpl for n, m in shapes), rpl
    assert {64, 65, 128, 129, 256, 257} <= {min(n, m) for n, m in shapes}
    # strip boundaries of the eight-row class other than 513: one strip exactly, two exactly, and one row more
    assert {512, 513, 1024, 1025} <= {min(n, m) for n, m in shapes}
    # and the split at 1 MiB has several sub-batches, some of one job over the budget
    subs = tc.split(shapes, tc.MIB)
    print("EDGE at 1 MiB:", len(subs), "sub-batches of", [c for _, c in subs])
    assert len(subs) >= 6 and any(c == 1 and tc.dir_bytes_for(*shapes[b]) > tc.MIB for b, c in subs)


def test_oracle_paths_are_shared_and_read_only(oracle):
    a, b = tc.oracle_paths(oracle, "edge"), tc.oracle_paths(oracle, "edge")
    assert a is b and not a[0][1].flags.writeable
    c, pi, pj, pd = a[0]
    assert pi[0] == 0 and pj[0] == 0 and len(pi) == len(pj) == len(pd)
