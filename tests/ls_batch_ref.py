"""Cases and reference for the DIRECT tests of eaqhm_ls_batch (tests/test_ls_batch_cases_cpu.py without a GPU,
tests/test_gpu_ls_batch_direct.py on one).  CPU only: NumPy plus the oracle.

A case is everything one frame_prep + ls_batch call needs, built so that every system size and every edge of the slot
set-up is present BY CONSTRUCTION instead of by what speech happens to produce:

  S  sizes       every n = 1..51 (tile rows nt = (4n + 18) >> 4 = 1..13) plus 52, 56 (large class); per n the sixteen
                 last-chunk shapes (wl + 1) % 16; long windows (wl 400, 511) for n in {1, 8, 30, 51}; slot lists with holes
  G  gaps        n in {2, 12, 30, 36, 42, 46, 50, 54} x every branch of the gap bridging (GAP_KINDS), words counted from
                 the window start c - wl as prepare_slots counts them
  P  placement   track_t0 = 1500 (no multiple of 1024), frames on both ends of the resident window, zeros on both sides
                 of a 1024-sample chunk boundary, a slot that is zero over a whole chunk, one frame that starts one
                 sample before the resident window (dropped); P0: track_t0 = 0, a frame with c - wl = 0
  E  seeding     frame centres whose fm column is empty, with neighbours that see / do not see the seeded sample
  Z  mode 0      frame_K = 1..51, 52, 60 at 16 kHz; Z48: frame_K in {100, 151, 152, 170} at 48 kHz
  B  large only  Kmax = 80, n in {52..80}, wl up to 560 (N > 1024: no tile path), a window over two chunk boundaries

The signal of a segment is a harmonic sum that follows the segment's tracks (1/k amplitudes, AM and FM of a few per
cent shared with the tracks) but not exactly: it carries an amplitude modulation and a phase wobble of its own, so the
slopes of the LS solution are real quantities (about 1e-3 of the amplitudes per sample) and not rounding noise — the
bars of the tests are relative to the largest slope of a frame.  Noise lies 50 dB under the segment's signal.

The reference is tests/fake_backend.py (OracleBackend.frame_prep / ls_batch, the oracle's seams with inv()).  `systems`
rebuilds each frame's weighted basis the way oracle.eaqhm_ls / iqhm_ls do, for the conditioning check: the same normal
equations solved by inv(), by Cholesky and by QR least squares."""
import numpy as np
import torch

import eaqhm_oracle as O
from fake_backend import OracleBackend

SENTINEL = float("nan")
GAP_KINDS = ("lead", "trail", "one", "word", "two_words", "from_bit0", "to_bit63", "first", "last", "outside",
             "two_gaps", "all_slots")
S_SIZES = list(range(1, 52)) + [52, 56]
S_LONG = {1: (400, 511), 8: (400, 511), 30: (400, 511), 51: (400, 511)}
G_SIZES = (2, 12, 30, 36, 42, 46, 50, 54)
B_SIZES = (52, 60, 64, 72, 80)
Z16_K = list(range(1, 52)) + [52, 60]
Z48_K = (100, 151, 152, 170)
SINGLES = (1, 23, 35, 43, 47, 51, 52)


def tile_rows(n):
    """Tile rows of the system of a frame with n active slots: order 2 (2n + 1) plus the right-hand-side row."""
    return (4 * n + 18) >> 4


class _Builder:
    """Lays segments of signal and tracks one after the other on the time axis and collects frames."""

    def __init__(self, fs, Kmax, seed, mode=1):
        self.fs, self.Kmax, self.mode = fs, Kmax, mode
        self.rng = np.random.default_rng(seed)
        self.s, self.am, self.fm = [], [], []
        self.pos = 0
        self.frames = []            # (c, wl, f0, K, tag)

    def silence(self, length):
        """No tracks, noise only."""
        if length <= 0:
            return self.pos
        self.s.append(1e-5 * self.rng.standard_normal(length))
        if self.mode == 1:
            self.am.append(np.zeros((self.Kmax, length)))
            self.fm.append(np.zeros((self.Kmax, length)))
        b, self.pos = self.pos, self.pos + length
        return b

    def pad_to(self, pos):
        assert pos >= self.pos, (pos, self.pos)
        self.silence(pos - self.pos)

    def segment(self, length, slots, f0):
        """`length` samples in which exactly `slots` are active: slot k follows harmonic k + 1 of f0.  Returns its start."""
        rng, fs = self.rng, self.fs
        slots = np.asarray(slots, dtype=int)
        t = np.arange(length) / fs
        h = (slots + 1.0)[:, None]
        fm = h * f0 * (1 + 0.02 * np.sin(2 * np.pi * 2.5 * t + rng.uniform(0, 2 * np.pi)))[None, :]
        am = 0.05 / h * (1 + 0.04 * np.sin(2 * np.pi * 4.0 * t[None, :] + rng.uniform(0, 2 * np.pi, (len(slots), 1))))
        ph = 2 * np.pi * np.cumsum(fm, axis=1) / fs + rng.uniform(0, 2 * np.pi, (len(slots), 1))
        # the signal's own modulation on top of the tracks': 30 % AM at 9 Hz, 0.5 rad phase wobble at 6 Hz (3 Hz peak)
        a_sig = am * (1 + 0.3 * np.sin(2 * np.pi * 9.0 * t[None, :] + rng.uniform(0, 2 * np.pi, (len(slots), 1))))
        p_sig = ph + 0.5 * np.sin(2 * np.pi * 6.0 * t[None, :] + rng.uniform(0, 2 * np.pi, (len(slots), 1)))
        x = 0.01 + 2 * (a_sig * np.cos(p_sig)).sum(axis=0)
        x = x + np.std(x) * 10 ** (-50 / 20) * rng.standard_normal(length)
        self.s.append(x)
        if self.mode == 1:
            A = np.zeros((self.Kmax, length))
            F = np.zeros((self.Kmax, length))
            A[slots], F[slots] = am, fm
            self.am.append(A)
            self.fm.append(F)
        b, self.pos = self.pos, self.pos + length
        return b

    def frame(self, c, wl, f0=0.0, K=0, **tag):
        self.frames.append((int(c), int(wl), float(f0), int(K), tag))

    def finish(self, name, track_t0=0, track_len=None, a_iter=1, f0_stale=200.0, f0min=160.0, dropped=0, sort=True):
        """`dropped`: the last `dropped` frames break the window contract on purpose (they stay last)."""
        self.silence(8)
        s = np.concatenate(self.s)
        L = len(s)
        fr = self.frames
        if sort:
            keep = fr[:len(fr) - dropped]
            fr = sorted(keep, key=lambda q: q[0]) + fr[len(fr) - dropped:]
        nf = len(fr)
        case = dict(name=name, mode=self.mode, fs=self.fs, L=L, Kmax=self.Kmax, s=s, n_frames=nf, dropped=dropped,
                    frame_c=np.array([q[0] for q in fr], dtype=np.int32),
                    frame_wl=np.array([q[1] for q in fr], dtype=np.int32),
                    frame_f0=np.array([q[2] for q in fr], dtype=np.float64),
                    frame_K=np.array([q[3] for q in fr], dtype=np.int32),
                    # record rows: one per frame, and three rows (first, middle, last) that no frame writes
                    frame_inst=(1 + np.arange(nf) + (np.arange(nf) >= nf // 2)).astype(np.int32), n_rows=nf + 3,
                    wl_max=int(max(q[1] for q in fr)), a_iter=a_iter, f0_stale=f0_stale, f0min=f0min,
                    tags=[dict(q[4], wl=q[1]) for q in fr])
        if self.mode == 1:
            am, fm = np.concatenate(self.am, axis=1), np.concatenate(self.fm, axis=1)
            track_len = L - track_t0 if track_len is None else track_len
            case.update(track_t0=track_t0, track_len=track_len, am_full=am, fm_full=fm,
                        am=np.ascontiguousarray(am[:, track_t0:track_t0 + track_len]),
                        fm=np.ascontiguousarray(fm[:, track_t0:track_t0 + track_len]))
            for f, tag in enumerate(case["tags"]):
                n = int(np.count_nonzero(fm[:, case["frame_c"][f]]))
                tag.setdefault("seeded", n == 0)
                tag["n"] = max(n, 1)
                tag["nt"] = tile_rows(tag["n"])
                tag.setdefault("gap", "none")
        else:
            case.update(track_t0=0, track_len=L, am=None, fm=None)
            for f, tag in enumerate(case["tags"]):
                tag["n"] = int(case["frame_K"][f])
                tag["nt"] = tile_rows(tag["n"])
                tag["gap"] = "none"
        return case


def _retag(case):
    """Sizes of the frames after zeros were put into the tracks (a slot that is zero on a frame's centre leaves it)."""
    for tag, c in zip(case["tags"], case["frame_c"]):
        n = int(np.count_nonzero(case["fm_full"][:, c]))
        tag["seeded"], tag["n"] = n == 0, max(n, 1)
        tag["nt"] = tile_rows(tag["n"])
    return case


def _punch(case, zero):
    """Zero the frequency tracks on (slot, lo, hi) ranges.  The amplitude tracks get wrong, nonzero values there: gap
    positions are decided on fm alone (functions.py:251-278), and an amplitude read from a gap shows in the solution."""
    t0, tl = case["track_t0"], case["track_len"]
    for k, lo, hi in zero:
        case["fm_full"][k, lo:hi] = 0.0
        case["am_full"][k, lo:hi] *= 3.0
    case["fm"] = np.ascontiguousarray(case["fm_full"][:, t0:t0 + tl])
    case["am"] = np.ascontiguousarray(case["am_full"][:, t0:t0 + tl])
    return _retag(case)


def _slots(rng, n, Kmax, holes):
    """n active slots; with `holes` they are drawn from a wider range so that the cols list is not 0..n-1."""
    if not holes or n >= Kmax:
        return np.arange(n)
    span = min(Kmax, n + max(2, n // 4))
    return np.sort(rng.choice(span, n, replace=False))


def _f0_for(slots, fs, cap=300.0):
    """Pitch whose highest active harmonic stays 400 Hz under Nyquist."""
    return min(cap, (fs / 2 - 400.0) / (int(np.max(slots)) + 1))


def _wl(fs, f0):
    return max(120, int(round(1.5 * fs / f0)))            # functions.py:191 with three pitch periods


# ------------------------------------------------------------------------------------------------ the sets
def case_S(seed=1):
    fs, Kmax = 16000, 56
    b = _Builder(fs, Kmax, seed)
    b.silence(16)
    for n in S_SIZES:
        slots = _slots(b.rng, n, Kmax, holes=(n % 5) in (0, 2, 3))
        f0 = _f0_for(slots, fs)
        wl0 = _wl(fs, f0)
        wls = [wl0 + r for r in range(16)] + list(S_LONG.get(n, ()))
        step = 3
        length = 2 * max(wls[:16]) + 1 + step * 16 + 8
        st = b.segment(length, slots, f0)
        for i, wl in enumerate(wls[:16]):
            b.frame(st + 2 + max(wls[:16]) + step * i, wl, holes=bool(np.any(np.diff(slots) > 1) or slots[0] > 0))
        for wl in wls[16:]:
            st = b.segment(2 * wl + 9, slots, f0)
            b.frame(st + wl + 4, wl, holes=bool(np.any(np.diff(slots) > 1) or slots[0] > 0), long=True)
    return b.finish("S", sort=False)


def _gap_ranges(kind, wl):
    """Zeroed ranges [lo, hi) in window offsets (0 = sample c - wl) of the ONE gappy slot; wl in 192..255, so the centre
    lies in word 3 and words 1-2 are whole and clear of it."""
    N = 2 * wl + 1
    assert 192 <= wl <= 255
    return {"lead": [(0, 37)], "trail": [(N - 29, N)], "one": [(70, 71)], "word": [(64, 128)],
            "two_words": [(64, 192)], "from_bit0": [(128, 150)], "to_bit63": [(100, 128)], "first": [(0, 1)],
            "last": [(N - 1, N)], "outside": [(-1, 0)], "two_gaps": [(30, 40), (300, 320)]}[kind]


def case_G(seed=2):
    fs, Kmax = 16000, 56
    b = _Builder(fs, Kmax, seed)
    b.silence(16)
    zero = []                                              # (slot, lo, hi) absolute
    for i, n in enumerate(G_SIZES):
        slots = _slots(b.rng, n, Kmax, holes=i % 2 == 1)
        f0 = _f0_for(slots, fs, cap=120.0)
        for j, kind in enumerate(GAP_KINDS):
            wl = 196 + (5 * i + 3 * j) % 56
            st = b.segment(2 * wl + 9, slots, f0)
            c = st + wl + 4
            w0 = c - wl
            if kind == "all_slots":
                for q, k in enumerate(slots):
                    lo = 8 + (37 * q) % (wl - 40)
                    zero.append((k, w0 + lo, w0 + lo + 1 + q % 9))
                    if q % 3 == 0:
                        zero.append((k, c + 20 + q, c + 20 + q + 2 + q % 70))
            else:
                k = slots[(7 * j + i) % n]
                for lo, hi in _gap_ranges(kind, wl):
                    zero.append((k, w0 + lo, w0 + hi))
            b.frame(c, wl, gap=kind)
    return _punch(b.finish("G", sort=False), zero)


def case_P(seed=3):
    """Resident window [1500, 7700) of a longer file."""
    fs, Kmax, t0, tlen = 16000, 56, 1500, 6200
    b = _Builder(fs, Kmax, seed)
    slots_a = _slots(b.rng, 12, Kmax, holes=True)
    slots_b = np.arange(40)
    f0a, f0b = _f0_for(slots_a, fs, cap=150.0), _f0_for(slots_b, fs)
    b.segment(3000, slots_a, f0a)                          # [0, 3000)
    b.segment(2000, slots_b, f0b)                          # [3000, 5000)
    b.segment(4000, slots_a, f0a)                          # [5000, 9000)
    wl = 170
    b.frame(t0 + 1 + wl, wl, place="first")                # c - wl - 1 == track_t0
    b.frame(t0 + 2 + wl, wl + 1, place="first")
    b.frame(t0 + tlen - 1 - 200, 200, place="last")        # c + wl == track_t0 + track_len - 1
    for c in (1900, 2047, 2048, 2100, 2200):               # windows that straddle sample 2048, zeros on 2047 and 2048
        b.frame(c, 180, place="straddle", gap="boundary")
    # slot 3 of the middle segment is zero over the whole chunk [3072, 4096)
    b.frame(4096 + 151, 151, place="chunk_after")          # c - wl - 1 == 4095: subtracts the count 1024
    b.frame(4096 + 130, 200, place="chunk_lead", gap="lead")   # a1 inside the zero chunk, b in the next: adds ztot = 1024
    b.frame(3071 - 140, 140, place="chunk_before")         # c + wl == 3071
    b.frame(3500, 130, place="chunk_inside")               # slot 3 inactive here: the window lies inside the zero chunk
    b.frame(t0 - 1 + wl, wl, place="dropped")              # c - wl == track_t0 - 1: not resident, dropped
    case = b.finish("P", track_t0=t0, track_len=tlen, dropped=1)
    k = int(slots_a[4])
    assert case["fm_full"][k, 2047] != 0 and case["fm_full"][3, 3500] != 0
    case["boundary_slot"], case["chunk_slot"] = k, 3
    case["side_slots"] = (int(slots_a[1]), int(slots_a[8]))
    return _punch(case, [(k, 2047, 2049),
                         (int(slots_a[1]), 2047, 2048),    # only the last sample of a chunk: seen through that chunk's counts alone
                         (int(slots_a[8]), 2048, 2049),    # only the first sample of the next
                         (3, 3072, 4096)])                 # (slot 3 leaves the frame at 3500)


def case_P0(seed=4):
    """Second launch of the placement set: track_t0 = 0, a window that starts on sample 0, zeros on the absolute samples
    1023 and 1024; f0_stale below f0min (the branch of functions.py:321 that leaves the frequency uncorrected)."""
    fs, Kmax = 16000, 56
    b = _Builder(fs, Kmax, seed)
    slots = _slots(b.rng, 20, Kmax, holes=True)
    b.segment(2600, slots, _f0_for(slots, fs))
    b.frame(150, 150, place="zero")                        # c - wl == 0
    b.frame(151, 150, place="one")                         # c - wl - 1 == 0
    for c in (900, 1023, 1024, 1100):
        b.frame(c, 160, place="straddle", gap="boundary")
    case = b.finish("P0", f0_stale=150.0, f0min=160.0)
    case["boundary_slot"], case["side_slots"] = int(slots[7]), (int(slots[2]), int(slots[13]))
    return _punch(case, [(int(slots[7]), 1023, 1025),
                         (int(slots[2]), 1023, 1024), (int(slots[13]), 1024, 1025)])   # one side of the boundary only, a slot each


def case_E(seed=5):
    fs, Kmax = 16000, 56
    b = _Builder(fs, Kmax, seed)
    b.silence(400)
    sa = np.arange(12)                                     # slot 0 active
    st_a = b.segment(1500, sa, 180.0)
    b.silence(700)                                         # an unvoiced stretch: every row empty
    sb = np.arange(1, 9)                                   # slot 0 not active
    st_b = b.segment(1500, sb, 210.0)
    empty = []                                             # samples whose whole fm column is zero
    e1, e2 = st_a + 600, st_a + 615
    for c, role in ((e1 - 45, "seed_after_centre"), (e1 - 15, "seed_after_centre"), (e1, "seeded"), (e2, "seeded"),
                    (e2 + 15, "seed_before_centre"), (e2 + 60, "seed_before_centre"), (e2 + 400, "clear")):
        b.frame(c, 140 + (c % 7), role=role, slot0=True)
    empty += [e1, e2]
    u = st_a + 1500 + 350
    for c in (u, u + 15, u + 30):
        b.frame(c, 130 + (c % 5), role="seeded", slot0=False)   # inside the silence: n = 1, only seeded samples in the window
    e3 = st_b + 700
    for c, role in ((e3 - 30, "seed_after_centre"), (e3, "seeded"), (e3 + 30, "seed_before_centre")):
        b.frame(c, 150, role=role, slot0=False)
    empty.append(e3)
    case = b.finish("E")
    case["fm"][:, empty] = 0.0
    case["am"][:, empty] *= 3.0                            # (wrong on purpose, see _punch)
    case["fm_full"], case["am_full"] = case["fm"], case["am"]
    for tag in case["tags"]:
        tag["gap"] = "seed"
    case["empty"] = empty
    return _retag(case)


def _case_Z(name, fs, Kmax, Ks, seed):
    b = _Builder(fs, Kmax, seed, mode=0)
    b.silence(16)
    for K in Ks:
        for shrink in (0.985, 0.9):
            f0 = min(400.0, (fs / 2 - 200.0) / K) * shrink           # K f0 <= fs/2 - 200
            wl = _wl(fs, f0)
            st = b.segment(2 * wl + 9, np.arange(K), f0)
            b.frame(st + wl + 4, wl, f0=f0 * (1.0 + 0.002 * (shrink < 0.95)), K=K)   # second frame: pitch 0.2 % off
    return b.finish(name, a_iter=0, f0_stale=0.0, sort=False)


def case_Z16(seed=6):
    return _case_Z("Z16", 16000, 60, Z16_K, seed)


def case_Z48(seed=7):
    return _case_Z("Z48", 48000, 170, Z48_K, seed)


def case_B(seed=8):
    fs, Kmax = 16000, 80
    b = _Builder(fs, Kmax, seed)
    b.silence(16)
    zero = []
    for i, n in enumerate(B_SIZES):
        slots = _slots(b.rng, n, Kmax, holes=i % 2 == 0)
        f0 = _f0_for(slots, fs)
        wl0 = _wl(fs, f0)
        for wl in (wl0 + i, wl0 + 7 + i, 400 + 3 * i, 512, 560):
            st = b.segment(2 * wl + 9, slots, f0)
            b.frame(st + wl + 4, wl)
    # a window of N = 1031 over two chunk boundaries: a1 = c - wl - 1 in one chunk, c + wl two chunks further
    slots = _slots(b.rng, 60, Kmax, holes=True)
    f0 = _f0_for(slots, fs)
    base = ((b.pos + 1023) >> 10) << 10
    b.pad_to(base + 1000)
    st = b.segment(1100, slots, f0)
    c = base + 1536
    b.frame(c, 515, place="two_boundaries")
    assert (c - 516) >> 10 == (base >> 10) and (c + 515) >> 10 == (base >> 10) + 2 and st <= c - 516
    for kind, wl in (("two_boundaries_gap", 515), ("word", 250)):     # the two gappy frames
        if kind == "word":
            st = b.segment(2 * wl + 9, slots, f0)
            c = st + wl + 4
            zero.append((int(slots[11]), c - wl + 64, c - wl + 128))
            zero.append((int(slots[40]), c + 100, c + wl + 1))
        else:
            base = ((b.pos + 1023) >> 10) << 10
            b.pad_to(base + 1000)
            b.segment(1100, slots, f0)
            c = base + 1536
            zero.append((int(slots[5]), base + 1023, base + 1025))
            zero.append((int(slots[5]), base + 2040, base + 2049))
            zero.append((int(slots[15]), base + 1022, base + 1023))   # seen only through the first chunk's counts,
            zero.append((int(slots[9]), base + 1300, base + 1311))    # only through the middle chunk's total,
            zero.append((int(slots[21]), base + 2050, base + 2051))   # only through the last chunk's running count
        b.frame(c, wl, gap=kind)
    return _punch(b.finish("B", sort=False), zero)


BUILDERS = dict(S=case_S, G=case_G, P=case_P, P0=case_P0, E=case_E, Z16=case_Z16, Z48=case_Z48, B=case_B)


# ------------------------------------------------------------------------------------------------ running a case
def reorder(case, order):
    """The same frames in another queue order (frame tables permuted; tracks, signal and record rows as they are)."""
    order = np.asarray(order)
    out = dict(case)
    for key in ("frame_c", "frame_wl", "frame_f0", "frame_K", "frame_inst"):
        out[key] = np.ascontiguousarray(case[key][order])
    out["tags"] = [case["tags"][i] for i in order]
    out["n_frames"] = len(order)
    return out


def run(case, ctx=None):
    """frame_prep + ls_batch of one case: on `ctx` (an eaqhm_amd.hip.Context; its faults are read) or, without one, on
    the NumPy model.  Returns records [n_rows][3 Kmax + 1] (rows no frame wrote keep the NaN sentinel), raw_amp /
    raw_slope [n_frames][2 Kmax + 1] complex (NaN past a frame's Kc), ncol, cols and the fault counts."""
    be = OracleBackend() if ctx is None else ctx
    dev = be.device
    nf, K, L, mode = case["n_frames"], case["Kmax"], case["L"], case["mode"]
    live = nf - (case["dropped"] if ctx is None else 0)     # the model has no window check: it is not shown such frames

    def T(a, dtype=None):
        return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)

    s, am, fm = T(case["s"]), T(case["am"]), T(case["fm"])
    inst, c, wl = T(case["frame_inst"]), T(case["frame_c"]), T(case["frame_wl"])
    f0, fK = T(case["frame_f0"]), T(case["frame_K"])
    ncol = torch.zeros(nf, dtype=torch.int32, device=dev)
    cols = torch.zeros(nf * K, dtype=torch.int32, device=dev)
    seeded = torch.zeros(L, dtype=torch.uint8, device=dev)
    any_seed = torch.zeros(1, dtype=torch.int32, device=dev)
    rec = torch.full((case["n_rows"], 3 * K + 1), SENTINEL, dtype=torch.float64, device=dev)
    raw_a = torch.full((nf, 2 * (2 * K + 1)), SENTINEL, dtype=torch.float64, device=dev)
    raw_s = torch.full((nf, 2 * (2 * K + 1)), SENTINEL, dtype=torch.float64, device=dev)
    if mode == 1:
        be.frame_prep(fm, L, case["track_t0"], case["track_len"], K, c, nf, ncol, cols, seeded, any_seed)
    be.ls_batch(mode, s, L, case["fs"], am, fm, case["track_t0"], case["track_len"], K, inst, c, wl, f0, fK, ncol, cols,
                seeded, any_seed, live, case["wl_max"], case["a_iter"], case["f0_stale"], case["f0min"], rec, raw_a, raw_s)
    faults = None
    if ctx is not None:
        torch.cuda.synchronize()
        faults = ctx.ls_faults()
    cx = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(np.complex128)
    return dict(records=rec.cpu().numpy(), raw_amp=cx(raw_a), raw_slope=cx(raw_s), ncol=ncol.cpu().numpy(),
                cols=cols.cpu().numpy().reshape(nf, K), seeded=np.flatnonzero(seeded.cpu().numpy()), faults=faults)


def one_thread():
    """The systems here are small (order <= 682): BLAS threads only get in each other's way, by a factor of 70."""
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1)
    except ImportError:
        import contextlib
        return contextlib.nullcontext()


def frame_inputs(case, ref):
    """Per live frame of a mode-1 case: (f, signal window, AM, FM) as functions.py:284-285 hands them to
    eaqhmLS_complexamps — gap-filled windows of the active slots in [negative | DC | positive] order."""
    L, K, t0, tl = case["L"], case["Kmax"], case["track_t0"], case["track_len"]
    am, fm = np.full((L, K), np.nan), np.full((L, K), np.nan)
    am[t0:t0 + tl], fm[t0:t0 + tl] = case["am"].T, case["fm"].T
    seeds, sp = list(ref["seeded"]), 0
    for f in range(case["n_frames"] - case["dropped"]):
        c, wl = int(case["frame_c"][f]), int(case["frame_wl"][f])
        while sp < len(seeds) and seeds[sp] <= c:
            fm[seeds[sp], 0], am[seeds[sp], 0] = 140, 10e-4
            sp += 1
        fw, aw = O.gather_fill(fm, am, c, wl, ref["cols"][f, :ref["ncol"][f]])
        z = np.zeros((fw.shape[0], 1))
        yield (f, case["s"][c - wl:c + wl + 1], np.concatenate((aw[::-1], z, aw), axis=1),
               np.concatenate((-fw[::-1], z, fw), axis=1))


def systems(case, ref):
    """Per live frame: (f, Ew, ws) with Ew = w [E, nE] the weighted basis and ws = w s the weighted signal, formed as
    oracle._weighted_ls forms them (inv(Ew^H Ew) Ew^H ws is the reference solution)."""
    if case["mode"] == 1:
        fs = case["fs"]
        for f, sig, AM, FM in frame_inputs(case, ref):
            wl = (len(sig) - 1) // 2
            nn = np.arange(-wl, wl + 1, dtype=np.float64)[:, None]
            fan = np.cumsum(FM, axis=0)
            t = 2 * np.pi * (fan - fan[wl]) / fs
            E, w = (O.EPS_AM + AM) / (AM[wl][None, :] + O.EPS_AM) * (np.cos(t) + 1j * np.sin(t)), np.hamming(2 * wl + 1)
            yield f, w[:, None] * np.concatenate((E, nn * E), axis=1), w * sig
        return
    fs = case["fs"]
    for f in range(case["n_frames"]):
        c, wl, K0 = int(case["frame_c"][f]), int(case["frame_wl"][f]), int(case["frame_K"][f])
        nn = np.arange(-wl, wl + 1, dtype=np.float64)[:, None]
        t = (nn * 2 * np.pi * (np.arange(-K0, K0 + 1) * case["frame_f0"][f])[None, :]) / fs
        E, w = np.cos(t) + 1j * np.sin(t), np.blackman(2 * wl + 1)
        yield f, w[:, None] * np.concatenate((E, nn * E), axis=1), w * case["s"][c - wl:c + wl + 1]


def three_solves(Ew, ws):
    """The normal equations of one frame solved by inv() (the reference), by Cholesky, and the least-squares problem
    itself by QR: three roundings of the same numbers."""
    from scipy.linalg import cho_factor, cho_solve, qr, solve_triangular
    EwH = Ew.conj().T
    R, rhs = EwH @ Ew, EwH @ ws
    Q, U = qr(Ew, mode="economic")
    return np.linalg.inv(R) @ rhs, cho_solve(cho_factor(R), rhs), solve_triangular(U, Q.conj().T @ ws)


def frame_errors(got, ref, case):
    """Per live frame: (amplitude error, slope error), each the largest absolute difference over the frame's Kc columns
    relative to the frame's largest reference magnitude; inf where a value is missing (NaN) in `got`."""
    out = np.empty((case["n_frames"] - case["dropped"], 2))
    for f in range(len(out)):
        Kc = 2 * case["tags"][f]["n"] + 1
        for j, key in enumerate(("raw_amp", "raw_slope")):
            r, g = ref[key][f, :Kc], got[key][f, :Kc]
            e = np.abs(g - r).max() / np.abs(r).max()
            out[f, j] = e if np.isfinite(e) else np.inf
    return out
