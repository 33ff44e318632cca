"""The model of the continuous pitch track (eaqhm_amd.pitch -> eaqhm_viterbi_*): a NumPy restatement of DESIGN.md §13.1.
No GPU and no library here.

    forward(S, cost, unvoiced=None, tile=8) -> dict(bp int16[T, npc + 1], tilemap int16[ntiles, npc + 1],
                                                      last float64[npc + 1], q int32[T])
        unvoiced is None or (uv, vcost).  Float64, every operation rounded once: the recurrence has no product, its
        maxima are exact and its ties are decided by rule, so an implementation equals this one bit for bit.
    brute_force(S, cost, unvoiced=None) -> (best score, every path that reaches it): all (npc [+ 1]) ** T paths
    refine(S, q, pc, ntc, nftc, ptab, nf, dtype) -> dict(p, s, k, gap): swipe_ref.pick's refinement along the path q
    fill_unvoiced(p, voiced, default), raw_path(S), big_steps(q, npc, over=8), voicing_changes(voiced)
    cases(tile) -> the hand-made forward cases of tests/test_gpu_pitch_viterbi.py: (name, S, cost, unvoiced)
"""
import itertools

import numpy as np

import swipe_ref as R


def _order(W):
    """Offsets in the order the tie rule prefers them: 0, -1, +1, -2, +2 ..."""
    out = [0]
    for d in range(1, W + 1):
        out += [-d, d]
    return np.array(out, dtype=np.int64)


def forward(S, cost, unvoiced=None, tile=8):
    S = np.ascontiguousarray(S, dtype=np.float64)
    cost = np.asarray(cost, dtype=np.float64)
    npc, T = S.shape
    W = len(cost) - 1
    assert 0 <= W <= npc - 1
    offs = _order(W)
    idx = np.arange(npc)[:, None] + offs[None, :]                 # the candidate c' of every (c, offset)
    inside = (idx >= 0) & (idx < npc)
    idx_c = np.clip(idx, 0, npc - 1)
    cst = cost[np.abs(offs)][None, :]
    ntiles = -(-T // tile)
    bp = np.empty((T, npc + 1), dtype=np.int16)
    tilemap = np.empty((ntiles, npc + 1), dtype=np.int16)
    bp[0] = np.arange(npc + 1)
    D = S[:, 0].copy()
    U = -np.inf if unvoiced is None else np.float64(unvoiced[0])
    org = np.arange(npc + 1)
    rows = np.arange(npc)
    for t in range(1, T):
        cand = np.where(inside, D[idx_c] - cst, -np.inf)
        first = cand.argmax(axis=1)                                # the first maximum in preference order
        best = cand[rows, first]
        pred = idx[rows, first]
        from_u = npc
        if unvoiced is not None:
            uv, vcost = np.float64(unvoiced[0]), np.float64(unvoiced[1])
            alt = U - vcost
            take = alt > best
            best = np.where(take, alt, best)
            pred = np.where(take, npc, pred)
            m = int(D.argmax())
            enter = D[m] - vcost
            if enter > U:
                Un, from_u = enter, m
            else:
                Un = U
            U = Un + uv
        D = best + S[:, t]
        bp[t, :npc] = pred
        bp[t, npc] = from_u
        new = org[bp[t].astype(np.int64)]
        if t % tile == 0:                                          # the step into a new tile completes the map before
            tilemap[t // tile - 1] = new
            org = np.arange(npc + 1)
        else:
            org = new
    tilemap[ntiles - 1] = org
    last = np.append(D, U)
    end = int(D.argmax())
    if unvoiced is not None and U > D[end]:
        end = npc
    q = np.empty(T, dtype=np.int32)
    q[T - 1] = end
    for t in range(T - 1, 0, -1):
        q[t - 1] = bp[t, q[t]]
    return dict(bp=bp, tilemap=tilemap, last=last, q=q)


def path_from_tilemap(m, T, tile=8):
    """q at the tile boundaries from the tile maps alone, then the tiles from bp: what the backtrack kernels do."""
    npc = m["bp"].shape[1] - 1
    q = np.full(T, -1, dtype=np.int32)
    D, U = m["last"][:npc], m["last"][npc]
    s = npc if U > D.max() else int(D.argmax())
    q[T - 1] = s
    for k in range(len(m["tilemap"]) - 1, -1, -1):
        s = int(m["tilemap"][k, s])
        q[k * tile] = s
    for k in range(len(m["tilemap"])):
        b, e = k * tile, min(k * tile + tile, T - 1)
        s = int(q[e])
        for t in range(e, b + 1, -1):
            s = int(m["bp"][t, s])
            q[t - 1] = s
    return q


def brute_force(S, cost, unvoiced=None):
    """Exact on inputs whose sums are exact (a dyadic grid): the best total and all paths with it."""
    npc, T = S.shape
    W = len(cost) - 1
    states = range(npc + (unvoiced is not None))
    best, paths = -np.inf, []
    for path in itertools.product(states, repeat=T):
        total, ok = 0.0, True
        for t, c in enumerate(path):
            total += unvoiced[0] if c == npc else S[c, t]
            if t:
                a = path[t - 1]
                if a == npc or c == npc:
                    total -= 0.0 if a == c else unvoiced[1]
                elif abs(a - c) > W:
                    ok = False
                    break
                else:
                    total -= cost[abs(a - c)]
        if not ok:
            continue
        if total > best:
            best, paths = total, [path]
        elif total == best:
            paths.append(path)
    return best, paths


def score(path, S, cost, unvoiced=None):
    npc = S.shape[0]
    total = 0.0
    for t, c in enumerate(path):
        total += unvoiced[0] if c == npc else S[c, t]
        if t:
            a = path[t - 1]
            if a == npc or c == npc:
                total -= 0.0 if a == c else unvoiced[1]
            else:
                total -= cost[abs(a - c)]
    return total


def refine(S, q, pc, ntc, nftc, ptab, nf, dtype=np.float64):
    """swipe_ref.pick's refinement (its closed form in long double, numpy.polyfit in float64 as swipep) of candidate q[t]
    at every instant; an edge candidate gives (pc[c], S[c, t]), the unvoiced state (0, 0).  gap: best minus runner-up
    over the fine grid (inf where there is no decision)."""
    npc, T = S.shape
    Sd = S.astype(dtype)
    p, s = np.zeros(T), np.zeros(T, dtype=dtype)
    kbest, gap = np.full(T, -1), np.full(T, np.inf)
    for it in range(T):
        i = int(q[it])
        if i >= npc:
            continue
        if i == 0 or i == npc - 1:
            p[it], s[it] = pc[i], Sd[i, it]
            continue
        x = ntc[i].astype(dtype)
        y = Sd[i - 1:i + 2, it]
        if dtype == np.float64:
            c = np.polyfit(x, y, 2)
        else:
            d01, d12 = (y[1] - y[0]) / (x[1] - x[0]), (y[2] - y[1]) / (x[2] - x[1])
            c2 = (d12 - d01) / (x[2] - x[0])
            c = (c2, d01 - c2 * (x[0] + x[1]), y[0] - x[0] * (d01 - c2 * x[1]))
        xf = nftc[i, :nf[i]].astype(dtype)
        val = np.zeros(len(xf), dtype=dtype)
        for ck in c:
            val = val * xf + ck
        k = int(val.argmax())
        others = np.delete(val, k)
        kbest[it], s[it], p[it] = k, val[k], ptab[i, k]
        gap[it] = float(val[k] - others.max()) if len(others) else np.inf
    return dict(p=p, s=s, k=kbest, gap=gap)


def fill_unvoiced(p, voiced, default):
    """Instant by instant: the nearest earlier voiced pitch, else the next later one, else `default`."""
    out = np.empty(len(p))
    held, first = None, None
    for t in range(len(p)):
        if voiced[t]:
            held = p[t]
            first = t if first is None else first
        out[t] = default if held is None else held
    if first is not None:
        out[:first] = p[first]
    return out


def raw_path(S):
    return S.argmax(axis=0)


def big_steps(q, npc, over=8):
    """Steps of more than `over` candidates between neighbouring voiced instants."""
    q = np.asarray(q, dtype=np.int64)
    both = (q[1:] < npc) & (q[:-1] < npc)
    return int((np.abs(np.diff(q))[both] > over).sum())


def voicing_changes(voiced):
    return int((np.diff(np.asarray(voiced, dtype=np.int8)) != 0).sum())


def cases(tile=8):
    """(name, S, cost, unvoiced): the hand-made inputs of the GPU test.  Every npc of the issue's list meets every T and
    every W somewhere; the big ones only with a few T so that the whole list stays quick."""
    out = []
    Ts = (1, 2, tile - 1, tile, tile + 1, 3 * tile + 5)
    for n, npc in enumerate((3, 63, 64, 65, 273, 1024)):
        Ws = sorted({0, 1, min(48, npc - 1), min(npc - 1, 256)})
        for a, T in enumerate(Ts):
            for b, W in enumerate(Ws):
                if npc >= 273 and (a + b + n) % 3:                 # a third of the big grid: each T and each W still occur
                    continue
                rng = np.random.default_rng(1000 * npc + 10 * T + W)
                kind = (a + b + n) % 4
                if kind == 0:
                    S = rng.uniform(-1, 1, (npc, T))
                else:
                    S = rng.integers(0, 8 if kind == 1 else 1024, (npc, T)) / 1024.0      # ties really occur
                if kind == 3 and T > 1:                            # maxima pinned to both candidate edges
                    S[0, ::2] = 2.0
                    S[-1, 1::2] = 2.0
                table = (a + b) % 3
                if table == 0:
                    cost = np.zeros(W + 1)
                elif table == 1:
                    cost = np.arange(W + 1) / 64.0
                else:
                    cost = np.maximum(0, np.arange(W + 1) - 2) / 32.0
                for unvoiced in (None, (0.25, 0.5), (-64.0, 0.25), (64.0, 0.25))[:4 if (a + b) % 2 == 0 else 2]:
                    tag = "off" if unvoiced is None else "uv%g" % unvoiced[0]
                    out.append(("npc%d-T%d-W%d-k%d-c%d-%s" % (npc, T, W, kind, table, tag), S, cost, unvoiced))
    # the unvoiced state entered at t = 0 and left at T - 1; left after t = 0; never entered although cheap to hold
    T = 2 * tile + 3
    S = np.full((5, T), 0.125)
    S[2, -1] = 4.0
    out.append(("entered-at-0-left-at-end", S.copy(), np.zeros(2), (0.5, 0.25)))
    S = np.full((5, T), 0.125)
    S[3, 1:] = 1.0
    out.append(("left-after-0", S.copy(), np.arange(3) / 8.0, (0.5, 0.25)))
    out.append(("zero-voicing-cost", np.random.default_rng(5).integers(0, 4, (7, T)) / 4.0, np.arange(4) / 16.0, (0.5, 0.0)))
    return out
