"""The context options on a live context: set then get against the record of the setter before the table (tests/option_cases.py), and the
environment's ways in -- RAWDTW_OPTS and the older spellings -- in fresh child processes.  Contexts only: no kernel runs."""
import json
import os
import subprocess
import sys

import pytest

import rawalign_amd as ra
from rawalign_amd._lib import RawDTWError
from tests import option_cases as oc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def live_context_sets_and_gets_as_recorded():
    """every option at three recorded values: -1, 1 and the last one recorded for it (its highest bound plus one, or the largest value there is)"""
    eng = ra.Engine(0)
    for name, cases in oc.CASES.items():
        assert eng.get_option(name) == oc.DEFAULTS[name], name
        picked = [c for c in cases if c[0] in (-1, 1)] + [cases[-1]]
        assert len({c[0] for c in picked}) == 3, name
        for value, status, stored, err in picked:
            eng.set_option(name, oc.DEFAULTS[name])   # (the record is of a fresh context: back to the default, which every option admits)
            assert eng.get_option(name) == oc.DEFAULTS[name], name
            if status == 0:
                eng.set_option(name, value)
            else:
                with pytest.raises(RawDTWError) as e:
                    eng.set_option(name, value)
                assert e.value.status == status and str(e.value) == "rawdtw status %d: %s" % (status, err), (name, value)
            assert eng.get_option(name) == stored, (name, value)
    for name, (status, err) in oc.REFUSED.items():
        with pytest.raises(RawDTWError) as e:
            eng.set_option(name, 1)
        assert e.value.status == status and str(e.value) == "rawdtw status %d: %s" % (status, err), name
    for name in oc.READ_ONLY:   # (nothing has run on this context)
        assert eng.get_option(name) == 0, name
    eng.close()


def child_options(env, names):
    """the options `names` of a context created in a fresh process under `env`"""
    code = "import json, rawalign_amd as ra; e = ra.Engine(0); print(json.dumps({n: e.get_option(n) for n in %r})); e.close()" % (names,)
    drop = ("RAWDTW_OPTS", "RAWDTW_LANE_HI", "RAWDTW_LANE_HI_MAX_N", "RAWDTW_LANE_MAX_R")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**{k: v for k, v in os.environ.items() if k not in drop}, **env},
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr   # (creation succeeded)
    return json.loads(run.stdout.strip().splitlines()[-1])


def rawdtw_opts_ignores_what_the_setter_refuses():
    got = child_options({"RAWDTW_OPTS": "sort_n=17,no_such=1,signal_cigar=2,lane_hi=1"}, ["sort_n", "lane_hi", "signal_cigar", "sort_r1_n"])
    assert got == {"sort_n": 17, "lane_hi": 1, "signal_cigar": 0, "sort_r1_n": oc.DEFAULTS["sort_r1_n"]}


def older_spellings_go_through_the_setter():
    stored = {value: s for value, _, s, _ in oc.CASES["lane_max_radius"]}
    assert stored[-2**63] == stored[-1]   # (-3 lies between two recorded values that the clamp takes to the same one)
    got = child_options({"RAWDTW_LANE_HI_MAX_N": "500", "RAWDTW_LANE_MAX_R": "-3"}, ["lane_hi_max_n", "lane_max_radius", "lane_hi"])
    assert got == {"lane_hi_max_n": 200, "lane_max_radius": stored[-1], "lane_hi": oc.DEFAULTS["lane_hi"]}


def test_options_on_a_live_context():
    live_context_sets_and_gets_as_recorded()
    rawdtw_opts_ignores_what_the_setter_refuses()
    older_spellings_go_through_the_setter()
