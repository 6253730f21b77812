"""Randomised pinning of the oracle against the REFERENCE ITSELF.

The reference's own ``take_turn`` / ``Agent.transition`` / ``Gridworld.move`` / ``visual_field`` were driven through
``oracle/make_golden.py``'s plugin classes on random shapes, agent counts, radii, rates, seeds and env ids
(``make_golden.random_case``), and every array they produced is stored under ``tests/golden/vs_reference/``
(``python -m oracle.make_golden vs_reference`` regenerates them where the reference tree is present).  Each case is
compared here with the Python restatement.
"""
import os

import numpy as np
import pytest

from oracle import make_golden as G


def _check(kind, case):
    spec, ids, turns, _run_kw, check_kw = G.random_case(kind, case)
    with np.load(os.path.join(G.VS_REFERENCE_DIR, f"{kind}_{case}.npz")) as d:
        out = {k: d[k] for k in d.files}
    assert str(out.pop("spec_json")) == G.spec_to_json(spec) and out.pop("env_ids").tolist() == ids, "the stored case is not this case"
    G.check_against_oracle(spec, ids, turns, out, **check_kw)


@pytest.mark.parametrize("case", range(10))
def test_treasurehunt_random_configs_match_the_reference(case):
    _check("treasurehunt", case)


@pytest.mark.parametrize("case", range(4))
def test_tag_random_configs_match_the_reference(case):
    _check("tag", case)


@pytest.mark.parametrize("case", range(3))
def test_cleanup_random_configs_match_the_reference(case):
    _check("cleanup", case)
