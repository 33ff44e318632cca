"""CPU tests of the two helpers the layers of eaqhm_amd.convert share: records._agree, the one check of a size the
library reports against its host mirror, and mapping._nonempty_rows / _put_rows, the empty-row and level bookkeeping of
conversion_apply and of the trajectory conversion.  No GPU, no library load."""
import numpy as np
import pytest

# the five messages as they were raised before there was a helper, character for character
DISAGREEMENTS = (
    "libeaqhm_hip.so and the host disagree on the size of the M-step's work buffer",
    "libeaqhm_hip.so and the host disagree on the size of the k-means update's work buffer",
    "libeaqhm_hip.so and the host disagree on the size of the trajectory solve's work buffer",
    "libeaqhm_hip.so and the host disagree on the size of the global-variance ascent's work buffer",
    "libeaqhm_hip.so and the host disagree on the splits of the nearest-row search",
)
PREFIX = "libeaqhm_hip.so and the host disagree on "


@pytest.mark.parametrize("message", DISAGREEMENTS)
def test_agree_raises_the_recorded_message(message):
    from eaqhm_amd.records import _agree
    what = message[len(PREFIX):]
    assert message == PREFIX + what
    for lib, host in ((1, 2), (2 ** 40, 2 ** 40 + 1), ((5, 64), (5, 128)), ((4, 64), (5, 64)), (-1, 0)):
        with pytest.raises(RuntimeError) as e:
            _agree(what, lib, host)
        assert str(e.value) == message
    for same in (0, 7, 2 ** 40, (5, 64)):
        assert _agree(what, same, same) is None


def test_every_disagreement_goes_through_agree():
    """The sentence is written once in the package, in records._agree, and each of the five places names its buffer."""
    import os
    from conftest import ROOT
    package = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd")
    text = {f: open(os.path.join(package, f)).read() for f in sorted(os.listdir(package)) if f.endswith(".py")}
    assert [f for f, s in text.items() if "the host disagree" in s] == ["records.py"]
    where = ("mixture.py", "mixture.py", "convert.py", "convert.py", "nonparallel.py")
    for message, f in zip(DISAGREEMENTS, where):
        assert '_agree("%s"' % message[len(PREFIX):] in text[f], (f, message)


EMPTY = np.array([-np.inf, 0.0, 0.0])
ROW = np.array([0.5, -1.0, 2.0])
CASES = dict(all_empty=[EMPTY, EMPTY, EMPTY], one_between=[EMPTY, ROW, EMPTY], none_empty=[ROW, 2 * ROW])


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_empty_row_bookkeeping(case, skip):
    from eaqhm_amd.mapping import _nonempty_rows, _put_rows
    C = np.array(CASES[case])
    width = 4                                             # the result is wider than the source: dy != dx
    full, rows, out = _nonempty_rows(C, width, skip)
    # the five steps in NumPy
    want_full = C[:, 0] != -np.inf
    want = np.zeros((len(C), width + skip))
    want[~want_full, 0] = -np.inf
    assert np.array_equal(full, want_full) and full.dtype == bool
    assert np.array_equal(rows, C[want_full][:, skip:]) and rows.shape == (want_full.sum(), 3 - skip)
    assert rows.flags["C_CONTIGUOUS"] and rows.dtype == np.float64
    assert np.array_equal(out, want) and out.shape == (len(C), width + skip)
    Y = 10.0 + np.arange(len(rows) * width, dtype=np.float64).reshape(len(rows), width)
    want[want_full, skip:] = Y
    if skip:
        want[want_full, 0] = C[want_full, 0]
    before = C.copy()
    got = _put_rows(out, full, skip, C, Y)
    assert got is out and np.array_equal(got, want) and np.array_equal(C, before)
    assert np.all(np.isneginf(got[~want_full, 0])) and not got[~want_full, 1:].any()
