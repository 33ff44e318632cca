"""Hand-built models for the resynthesis kernels of csrc/eaqhm_modify.hip (prep, segmented scan, carry, the four eval
kernels) and the Python mirror of their launch geometry.  The CPU tests (test_modify_cases_cpu.py) show that the cases
hold what is claimed here; the GPU tests (test_gpu_modify_direct.py) run the kernels on them.

An analysed model never has a frequency order other than the slot order, an active instant 0, 1 or No_ti-1, a run placed
on a scan-chunk boundary on purpose, or a Kmax that selects the smaller blocks of the eval kernels.  These records are
written directly: [n, 3K+1], amplitudes and frequencies smooth along time, phases seeded uniform in (-pi, pi], an a0
column that is not zero, and an activity mask given pattern by pattern.  The slot order is a seeded permutation of the
frequency order unless a case says otherwise.

    cases() -> [dict(name, records, active, No_ti, Kmax, step, fs, L, settings, checks)]

L = (n-1) step + 1 + 133: at rho >= 1 the output runs two 64-sample blocks past the last knot (the a0 extrapolation
and blocks without any slot in a run).  `settings` is a list of (rho, beta, envelope); `checks` a list of
(label, slot, instant, run code) that names every pattern the case was built for.
"""
import numpy as np

SCAN_CH = 64                    # instants per chunk of eaqhm_modify_scan_kernel
CARRY_TILE = 64                 # chunks per tile of eaqhm_modify_carry_kernel
LDS_BUDGET = 78 * 1024

SETTINGS = [(1.0, 1.0, True), (0.25, 1.3, True), (4.0, 0.5, True), (0.7, 1.0, False), (1.5, 2.0, True)]
# `long` (63 119 samples) leaves the setting rho = 4 out: its four settings keep the largest output at 95 k samples, and
# the carry kernel's two tiles, which are what the case is for, do not depend on rho.
SETTINGS_LONG = [s for s in SETTINGS if s[0] != 4.0]


# --------------------------------------------------------------------------------------------- launch geometry
def modify_lds_bytes(K, step, tbs, nr, crow=0, shape=0):
    """LDS bytes of an eval block (csrc/eaqhm_modify.hip, modify_lds_bytes)."""
    return ((step + 2) & ~1) * 8 + K * (tbs + 1) * 8 + tbs * 8 + nr * ((3 * K + 1) + (K + 1)) * 8 + \
        ((tbs + 1) & ~1) * 4 + ((nr * K + 7) & ~7) + nr * crow * 8 + tbs * shape * 8


def modify_block_samples(K, step, rho, crow=0, shape=0):
    """(samples per block, staged rows, rows wanted, LDS bytes) of the eval kernels at the time map's smallest rate rho
    (modify_block_samples of the same file): the largest of 64 / 32 / 16 samples whose tables fit the budget with the
    staged rows cut down to no fewer than 4; 16 is taken even above the budget.  crow = 3 for the contour kernels,
    shape = 1 for the shape kernels."""
    for tbs in (64, 32, 16):
        want = int(np.ceil((tbs - 1) / (rho * step))) + 6
        nr = want
        while nr > 4 and modify_lds_bytes(K, step, tbs, nr, crow, shape) > LDS_BUDGET:
            nr -= 1
        b = modify_lds_bytes(K, step, tbs, nr, crow, shape)
        if b <= LDS_BUDGET or tbs == 16:
            return tbs, nr, want, b
    raise AssertionError


# --------------------------------------------------------------------------------------------- records
def _records(active, fs, rng, freq_rank=None, freq=None):
    """Records for an activity mask.  Slot k's frequency is 100 Hz + rank_k x spacing (spacing so that the top stays
    under 0.46 fs), 2 % slow modulation; amplitudes 10^-3 .. 1 with 40 % slow modulation; inactive cells all zero."""
    n, K = active.shape
    x = np.arange(n) / max(n - 1, 1)
    rec = np.zeros((n, 3 * K + 1))
    rank = np.arange(K) if freq_rank is None else freq_rank
    spacing = (0.45 * fs - 100.0) / K
    for k in range(K):
        level = 10.0 ** rng.uniform(-3, 0)
        am = level * (1.0 + 0.4 * np.sin(2 * np.pi * (rng.uniform(0.5, 3) * x + rng.uniform())))
        if freq is None:
            fm = (100.0 + rank[k] * spacing) * (1.0 + 0.02 * np.sin(2 * np.pi * (rng.uniform(0.5, 4) * x + rng.uniform())))
        else:
            fm = np.full(n, freq[k])
        ph = -rng.uniform(-np.pi, np.pi, n)                           # (-pi, pi]
        a = active[:, k]
        rec[a, k] = am[a]
        rec[a, K + k] = fm[a]
        rec[a, 2 * K + k] = ph[a]
    rec[:, 3 * K] = 0.02 + 0.01 * np.sin(2 * np.pi * 2.3 * x) + 0.003 * rng.standard_normal(n)
    return rec


def _case(name, active, step, fs, checks, seed, settings=SETTINGS, permute=True, freq=None):
    n, K = active.shape
    rng = np.random.default_rng([seed, n, K, step, int(fs)])
    rank = rng.permutation(K) if permute else np.arange(K)
    rec = _records(active, fs, rng, rank, freq)
    return dict(name=name, records=rec, active=active, No_ti=n, Kmax=K, step=step, fs=float(fs),
                L=(n - 1) * step + 1 + 133, settings=list(settings), checks=checks, freq_rank=rank)


def _short(m, pos):
    return 16 + 4 * m + pos


class _Mask:
    """Activity mask built pattern by pattern; every pattern leaves the run codes it stands for in `checks`."""

    def __init__(self, n, K):
        self.a = np.zeros((n, K), bool)
        self.checks = []

    def run(self, k, first, last, label=None):
        self.a[first:last + 1, k] = True
        m = last - first + 1
        if label:
            if m == 1:
                self.checks.append((label, k, first, 1))
            elif m >= 4:
                self.checks += [(label, k, first, 2), (label, k, last, 2)]
            else:
                self.checks += [(label, k, first + p, _short(m, p)) for p in range(m)]
        return self

    def off(self, k, i, label):
        self.checks.append((label, k, i, 0))
        return self


def chunks():
    n, K = 140, 70
    m = _Mask(n, K)
    m.run(0, 0, n - 1, "active throughout")
    m.off(1, 64, "never active")
    m.run(2, 40, 63, "run ending at 63").off(2, 64, "run ending at 63")
    m.run(3, 64, 90, "run starting at 64").off(3, 63, "run starting at 64")
    m.run(4, 63, 64, "2-run 63-64")
    m.run(5, 62, 65, "run 62-65")
    m.run(6, 64, 64, "isolated knot at 64")
    m.run(7, 0, 126, "gap at 127-128").run(7, 129, n - 1, "gap at 127-128").off(7, 127, "gap").off(7, 128, "gap")
    m.run(8, 0, 0, "isolated knot at 0").run(8, n - 1, n - 1, "isolated knot at n-1")
    m.run(9, n - 2, n - 1, "2-run ending at n-1")
    m.run(10, n - 3, n - 1, "3-run ending at n-1")
    # short runs behind an active start (the pad instants carry fm) and behind an empty one (they carry 0)
    m.run(11, 0, 5, "start active").run(11, 20, 20, "1-run, pad fm").run(11, 30, 31, "2-run, pad fm")
    m.run(11, 40, 42, "3-run, pad fm").run(11, 70, 71, "2-run, pad fm").run(11, 126, 128, "3-run over 127-128, pad fm")
    m.run(12, 20, 20, "1-run, pad 0").run(12, 30, 31, "2-run, pad 0").run(12, 40, 42, "3-run, pad 0")
    m.off(12, 0, "start empty").off(12, 1, "start empty").off(12, 2, "start empty")
    for k in range(13, 64):
        m.run(k, 0, n - 1)
    rng = np.random.default_rng(140070)
    for k in range(13, 64, 7):                                        # seeded gaps of 1-3 instants
        i = int(rng.integers(5, n - 8))
        m.a[i:i + int(rng.integers(1, 4)), k] = False
    # the second 64-lane pass of env_compact / env_rank, with gaps
    m.off(64, 64, "never active (slot 64)")
    m.run(65, 10, 50, "run 10-50 (slot 65)").off(65, 51, "run 10-50 (slot 65)")
    m.run(66, 0, n - 1, "active throughout (slot 66)")
    m.run(67, 0, 63, "cut at 64 (slot 67)").run(67, 65, n - 1, "cut at 64 (slot 67)").off(67, 64, "cut at 64 (slot 67)")
    m.run(68, 3, 3, "isolated knot at 3 (slot 68)").run(68, 64, 127, "run 64-127 (slot 68)")
    m.run(69, 0, n - 1, "active throughout (slot 69)")
    return _case("chunks", m.a, 15, 16000, m.checks, seed=1)


def _wide(name, K, seed):
    n = 12
    m = _Mask(n, K)
    for k in range(K):
        m.run(k, 0, n - 1)
    m.a[:, 1] = False
    m.off(1, 5, "never active")
    for k, pats in ((2, [(0, 0), (4, 5), (9, 11)]), (3, [(1, 3), (6, 6), (8, 9)]), (K - 1, [(2, 2), (5, 7), (10, 11)]),
                    (K // 2, [(0, 1), (5, 5), (7, 10)]), (65, [(3, 4), (7, 7), (9, 11)])):
        m.a[:, k] = False
        for a, b in pats:
            m.run(k, a, b, "slot %d: %d-%d" % (k, a, b))
    return _case(name, m.a, 15, 48000, m.checks, seed=seed)


def k150():
    return _wide("k150", 150, seed=2)


def k300():
    return _wide("k300", 300, seed=3)


def tiny():
    a = _Mask(4, 1).run(0, 0, 3, "one run of 4")
    b = _Mask(4, 1).run(0, 0, 2, "3-run at 0-2").off(0, 3, "3-run at 0-2")
    return [_case("tiny_run4", a.a, 15, 16000, a.checks, seed=4), _case("tiny_start3", b.a, 15, 16000, b.checks, seed=5)]


def step2():
    n, K = 40, 3
    m = _Mask(n, K)
    for i in range(0, n, 2):
        m.run(0, i, i, "isolated every 2")
    for i in range(1, n, 4):
        m.run(1, i, i, "isolated every 4")
    m.run(2, 0, 17, "run 0-17").run(2, 19, 20, "2-run 19-20").run(2, 22, 22, "isolated 22").run(2, 24, n - 1, "run to n-1")
    return _case("step2", m.a, 2, 16000, m.checks, seed=6)


def long():
    n, K = 4200, 3
    assert (n + SCAN_CH - 1) // SCAN_CH == 66 > CARRY_TILE
    m = _Mask(n, K)
    m.run(0, 0, n - 1, "active throughout")
    m.run(1, 7, 2000, "run 7-2000").run(1, 4096, n - 1, "run starting at 4096").off(1, 4095, "run starting at 4096")
    m.run(2, 100, 4095, "run ending at 4095").off(2, 4096, "run ending at 4095").run(2, 4150, 4151, "2-run 4150-4151")
    return _case("long", m.a, 15, 16000, m.checks, seed=7, settings=SETTINGS_LONG)


START_COLLIDING = {0: (0, 1), 1: (0, 2), 2: (1, 2)}         # slot: the run whose pad instants are its own knots
START_PLAIN = {3: (0, 0), 4: (1, 3), 5: (2, 3)}             # slot: start runs with four distinct nodes, or isolated


def start():
    n, K = 12, 6
    m = _Mask(n, K)
    for k, (a, b) in sorted({**START_COLLIDING, **START_PLAIN}.items()):
        m.run(k, a, b, "start run %d-%d" % (a, b))
        m.run(k, 6 + k % 2, n - 1 - k % 3, "later run")
    return _case("start", m.a, 15, 16000, m.checks, seed=8)


HARM_DUP = (6, 5)               # the slot of harmonic 7 (875 Hz) carries harmonic 6's frequency, 750 Hz, as well
HARM_SINGLE, HARM_NONE = 3, 5   # the instant with one active slot and the instant with none


def harm125():
    n, K = 8, 40
    rng = np.random.default_rng(125)
    slot_of = rng.permutation(K)                                      # slot_of[h]: the slot of harmonic h+1
    freq = np.zeros(K)
    freq[slot_of] = 125.0 * (np.arange(K) + 1)
    freq[slot_of[HARM_DUP[0]]] = freq[slot_of[HARM_DUP[1]]]
    m = _Mask(n, K)
    keep = int(slot_of[10])
    for k in range(K):
        if k == keep:
            m.run(k, 0, 4, "the slot of the single instant").run(k, 6, 7)
        else:
            m.run(k, 0, 2).run(k, 4, 4).run(k, 6, 7)
    m.off((keep + 1) % K, HARM_SINGLE, "single instant").off(keep, HARM_NONE, "empty instant")
    c = _case("harm125", m.a, 15, 16000, m.checks, seed=9, freq=freq)
    c["slot_of"] = slot_of
    return c


def cases():
    """The named cases (same seeds, same cases)."""
    return [chunks(), k150(), k300()] + tiny() + [step2(), long(), start(), harm125()]


def contour_scales(n):
    """The contour pair of the direct tests: rho = 0.25 + 0.5 x and beta = 1.3 - 0.5 x over the instants."""
    x = np.arange(n) / max(n - 1, 1)
    return 0.25 + 0.5 * x, 1.3 - 0.5 * x
