"""The resynthesis on the MI355X against the samples of the commit before the synthesis entry points were folded
(four eaqhm_modify_synth* into eaqhm_modify_synth, the modulated twin of eaqhm_noise_synth into it, ABI 6): sha256
digests of every case of tests/synth_parent_cases.py, recorded on the MI355X at the commit
tests/golden/synth_parent_digests.json names.  The cases run every arm of the two dispatches: both time maps, both
phase modes, the noise plain and modulated, written and accumulated, whole and in ranges."""
import json

import numpy as np
import pytest

import synth_parent_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return S.cases(eaqhm_amd, S.inputs(eaqhm_amd))


def test_every_case_is_the_parents_bit_for_bit(got):
    with open(S.FIXTURE) as f:
        want = json.load(f)
    assert set(got) == set(want["cases"])
    for key in sorted(got):
        assert S.digest(got[key]) == want["cases"][key], key


def test_ranges_give_the_whole_bit_for_bit(got):
    """Independent of the fixture: a synthesis computed in three uneven ranges is the one computed whole."""
    parts = [k for k in got if k.endswith(S.RANGES)]
    assert len(parts) == 8
    for key in parts:
        whole = got[key[:-len(S.RANGES)]]
        assert np.abs(whole).max() > 0 and np.array_equal(got[key], whole), key
