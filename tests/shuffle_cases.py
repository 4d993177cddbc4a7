"""What tests/test_shuffle_host.py (CPU) and tests/test_gpu_shuffle.py (GPU) share: a numpy model of the path choice of
k_fy_stream (csrc/lgcn_shuffle.hip), the stream cases it is started on, the J families fed to the swap resolution through
lgcn_fy_resolve_device, and a numpy restatement of that resolution.  Test infrastructure; everything here is integer and exact.

THE PATH MODEL (stream_ledger).  k_fy_stream walks two wave-uniform numbers, the Fisher-Yates step i (n-1 down to 1) and the read
position idx in the current 624-word block, and takes one of five paths per turn of its loop:

  fast             after a twist, when i - 624 >= max(FY_TAIL, low): the whole block, ten passes from registers, thresholds of
                   the block's first step (definite: draw <= i0 - 624; ambiguous: i0 - 624 < draw <= i0, resolved in order)
  reg              after a twist, otherwise: up to ten passes of 64 (the tenth: 48) draws from registers while i >= FY_TAIL and
                   i - 64 >= low, decided again before every pass
  lds              without a twist (idx < 624): one pass of min(64, 624 - idx) draws read back from LDS, same condition
  serial_boundary  idx < 624, i >= FY_TAIL, i - 64 < low: lane 0 alone down to step low (the mask changes below it) or to the end
                   of the block
  serial_tail      idx < 624, i < FY_TAIL: lane 0 alone down to step 1 or to the end of the block

with low = (mask >> 1) + 1, the smallest step that draws under the mask of step i, and FY_TAIL = 1024.  The model walks (i, idx)
in the same way over the raw MT19937 words numpy produces from the same state, with the same thresholds and the same in-order
resolution of the ambiguous draws, and keeps a ledger: the paths in order, every hand-over (previous path, whether a twist lies
between, next path) and the rare events listed in EVENTS.  Its J is pinned to numpy (the swap loop over it must give
RandomState.shuffle), so a ledger is a statement about numpy's stream, not about the kernel's output.

What the code permits (HANDOVERS) follows from three facts.  (1) A pass (fast, reg, lds) needs i - 64 >= low and i >= 1024 before it
and accepts at most 64 draws, so it leaves i >= max(low, 1024) under the SAME mask: the tail never follows a pass directly, and
the register passes of a block never cross a boundary.  (2) After a twist, `reg` with no pass at all is exactly the serial
condition, so a twist is never followed by `lds`.  (3) The fast guard can only fail for smaller i under one mask, so neither
the tenth register pass nor a cut serial stretch is followed by `fast`; a serial stretch that reaches its boundary 2^k at the
block's last word is (i = 2^k - 1 >= 2047 clears the guard; i = 1023 is the tail)."""
import collections

import numpy as np

MT_N, FY_TAIL = 624, 1024

# ---- the generator --------------------------------------------------------------------------------------------------------------
KEY_SOURCES = ((2020, 1000), (7, 12345))        # key id -> (seed, 32-bit draws taken before the key is read)


def make_key(kid):
    seed, burn = KEY_SOURCES[kid]
    rs = np.random.RandomState(seed)
    rs.randint(0, 2 ** 31, size=burn)
    return np.ascontiguousarray(rs.get_state()[1], np.uint32)


def _temper(y):
    y ^= y >> 11
    y ^= (y << 7) & 0x9d2c5680
    y ^= (y << 15) & 0xefc60000
    y ^= y >> 18
    return y & 0xffffffff


def _untemper(y):
    y ^= y >> 18
    y ^= (y << 15) & 0xefc60000
    y0 = y
    for _ in range(5):
        y = y0 ^ ((y << 7) & 0x9d2c5680)
    y0 = y
    for _ in range(3):
        y = y0 ^ (y >> 11)
    return y & 0xffffffff


def key_before_block(words):
    """A key whose NEXT block (state (key, 624): the first draw twists) outputs `words` [624] -- all but the low 31 bits of
    words[0]'s state word, which the twist ties to words 396 and 623.  -> (key uint32 [624], the words it really gives).
    MT19937's twist run backwards: new[i] = far ^ f(hi(old[i]) | lo(old[i+1])) with f(Y) = (Y >> 1) ^ (Y odd ? A : 0); A has its top
    bit set, so the top bit of f(Y) is Y's parity and Y follows; `far` is new[i - 227] for i >= 227 and old[i + 397] below."""
    A, HI, LO = 0x9908b0df, 0x80000000, 0x7fffffff
    new = [_untemper(int(w)) for w in words]

    def inv_f(y):
        return ((((y ^ A) << 1) | 1) if y & HI else (y << 1)) & 0xffffffff

    hi, lo = [0] * MT_N, [0] * MT_N
    Y = inv_f(new[623] ^ new[396])
    hi[623] = Y & HI
    new[0] = (new[0] & HI) | (Y & LO)             # the constraint: word 623 reads the NEW word 0
    for i in range(622, 226, -1):
        Y = inv_f(new[i] ^ new[i - 227])
        hi[i], lo[i + 1] = Y & HI, Y & LO
    for i in range(226, -1, -1):
        Y = inv_f(new[i] ^ (hi[i + 397] | lo[i + 397]))
        hi[i], lo[i + 1] = Y & HI, Y & LO
    key = np.asarray([h | l for h, l in zip(hi, lo)], np.uint32)
    return key, np.asarray([_temper(w) for w in new], np.int64)


def _crafted_all_accepted():
    """Every draw of the first block below 1024 under the mask 2047 (the high bits random): from step 1648, where the fast guard
    holds with equality, all 624 draws (623 if word 0 says so) are accepted and the block ends on step 1024 or 1025 -- the
    only way from the fast path straight into a serial stretch.  Draws from a seeded stream would need 561 acceptances of 624
    at a rate of two in three."""
    rng = np.random.Generator(np.random.PCG64(1648))
    words = (rng.integers(0, 1 << 21, MT_N) << 11) | rng.integers(0, 1024, MT_N)
    key, got = key_before_block(words)
    assert np.array_equal(got[1:], words[1:])
    return key


CRAFTED = {"all_accepted": _crafted_all_accepted}
_KEYS = {}


def key_of(kid):
    """kid: an index into KEY_SOURCES, or a name in CRAFTED (extra cases)."""
    if kid not in _KEYS:
        _KEYS[kid] = CRAFTED[kid]() if isinstance(kid, str) else make_key(kid)
    return _KEYS[kid]


def numpy_state(key, pos):
    rs = np.random.RandomState()
    rs.set_state(('MT19937', np.asarray(key, np.uint32), int(pos)))
    return rs


def numpy_shuffle(key, pos, n, tail=0):
    """(np.random.shuffle(arange(n)) from the state (key, pos), the next shuffle of arange(tail) on the same stream)."""
    rs = numpy_state(key, pos)
    perm = np.arange(n, dtype=np.int64)
    rs.shuffle(perm)
    more = np.arange(tail, dtype=np.int64)
    rs.shuffle(more)
    return perm, more


def raw_words(key, pos, count):
    """The next `count` raw 32-bit outputs of numpy's MT19937 from the state (key, pos)."""
    bg = np.random.MT19937()
    bg.state = {'bit_generator': 'MT19937', 'state': {'key': np.asarray(key, np.uint32), 'pos': int(pos)}}
    return bg.random_raw(int(count)).astype(np.int64)


def lib_set_state(lib, key, pos):
    key = np.ascontiguousarray(key, np.uint32)
    assert key.shape == (MT_N,)
    lib.lgcn_np_set_state(key.ctypes.data, int(pos))


def lib_get_state(lib):
    import ctypes as C
    key = np.zeros(MT_N, np.uint32)
    pos = C.c_uint32(0)
    lib.lgcn_np_get_state(key.ctypes.data, C.byref(pos))
    return key, int(pos.value)


TAIL = 700          # the continuation that is compared: a shuffle of arange(700) crosses at least one block boundary


# ---- the stream cases -----------------------------------------------------------------------------------------------------------
TOPS = [1, 2, 63, 64, 65, 1022, 1023, 1024, 1025, 1087, 1088, 1089, 1647, 1648, 1649]              # n - 1
TOPS += [(1 << k) + o for k in (11, 12, 16) for o in (-1, 0, 1, 63, 64, 65, 623, 624, 625)]
POS0 = [0, 1, 63, 64, 65, 560, 561, 575, 576, 577, 623, 624]
# (key id | name in CRAFTED, n - 1, pos0): what the grid above does not meet.  The grid meets every hand-over but
# one, fast -> twist -> serial_boundary, which no seeded stream reaches (_crafted_all_accepted says why): a key built for it.
EXTRA_CASES = [("all_accepted", 1648, MT_N)]


def stream_cases():
    """[(key id, n, pos0)], the grid of the issue and the named extras."""
    out = [(kid, top + 1, pos0) for kid in range(len(KEY_SOURCES)) for top in TOPS for pos0 in POS0]
    return out + [(kid, top + 1, pos0) for kid, top, pos0 in EXTRA_CASES]


def group_of(n):
    top = n - 1
    return "small" if top < 2000 else "2^11" if top < 4000 else "2^12" if top < 60000 else "2^16"


GROUPS = ("small", "2^11", "2^12", "2^16")

# ---- the path model -------------------------------------------------------------------------------------------------------------
PATHS = ("fast", "reg", "lds", "serial_boundary", "serial_tail")
# (previous path, a twist between them, next path): everything k_fy_stream's control flow permits (module docstring)
HANDOVERS = {
    ("start", 0, "lds"), ("start", 0, "serial_boundary"), ("start", 0, "serial_tail"),
    ("start", 1, "fast"), ("start", 1, "reg"), ("start", 1, "serial_boundary"), ("start", 1, "serial_tail"),
    ("fast", 1, "fast"), ("fast", 1, "reg"), ("fast", 1, "serial_boundary"),
    ("reg", 0, "reg"), ("reg", 0, "serial_boundary"), ("reg", 1, "reg"), ("reg", 1, "serial_boundary"),
    ("lds", 0, "lds"), ("lds", 0, "serial_boundary"), ("lds", 1, "fast"), ("lds", 1, "reg"), ("lds", 1, "serial_boundary"),
    ("serial_boundary", 0, "lds"), ("serial_boundary", 0, "serial_tail"),
    ("serial_boundary", 1, "fast"), ("serial_boundary", 1, "serial_boundary"), ("serial_boundary", 1, "serial_tail"),
    ("serial_tail", 1, "serial_tail"), ("serial_tail", 0, "end"),
}
GUARD_LOWS = (1024, 2048, 4096, 65536)          # the boundaries the grid puts the fast guard on: 1648 - 624 and 2^k for k = 11, 12, 16
EVENTS = {
    # two ambiguous draws in one pass; and, of those, a later one whose fate the earlier ones decide: it is accepted against the
    # count of the definite draws alone and rejected when every earlier ambiguous draw of the pass counts too (or the other way)
    ("two_ambiguous", "fast"), ("two_ambiguous", "pass"), ("ambiguous_depends", "fast"), ("ambiguous_depends", "pass"),
    "ragged_lds_pass",                          # c = 624 - idx < 64
    "ragged_tenth_register_pass",               # the 48 draws of words 576..623, pass by pass
    "serial_boundary_cut_by_block_end", "serial_tail_cut_by_block_end",
    "ends_on_block_end",                        # the call's last draw is word 623: the state goes back with idx == 624
    ("pass_guard_equal", "reg"), ("pass_guard_missed_by_one", "reg"),        # i - 64 == low and low - 1
    ("pass_guard_equal", "lds"), ("pass_guard_missed_by_one", "lds"),
} | {(name, low) for name in ("fast_guard_equal", "fast_guard_missed_by_one") for low in GUARD_LOWS}      # i - 624 == low, low - 1


def fy_mask(i):
    m = int(i)
    for s in (1, 2, 4, 8, 16):
        m |= m >> s
    return m


class Ledger:
    def __init__(self):
        self.paths = []                         # [[path, times in a row]]
        self.handovers = collections.Counter()
        self.events = collections.Counter()
        self.J = None
        self.draws = 0                          # words consumed
        self.final_idx = None

    def sequence(self, limit=60):
        """'lds x9, TWIST, fast x3, ...' for an assert message (the first and last `limit` / 2 runs)."""
        runs = [p if c == 1 else f"{p} x{c}" for p, c in self.paths]
        if len(runs) > limit:
            runs = runs[:limit // 2] + [f"... {len(runs) - limit} runs ..."] + runs[-limit // 2:]
        return ", ".join(runs)


def _resolve_pass(v, lanes_in, i, window, led, where):
    """The two ballots and the in-order resolution of one pass: draws v (already masked) of the lanes < lanes_in against step i,
    definite when v <= i - window.  -> bool [len(v)] accepted.  Records the ambiguity events under `where`."""
    inl = np.arange(len(v)) < lanes_in
    definite = inl & (v <= i - window)
    acc = definite.copy()
    amb = np.flatnonzero(inl & ~definite & (v <= i))
    if len(amb) >= 2:
        led.events[("two_ambiguous", where)] += 1
    ndef = np.cumsum(definite) - definite        # definite draws below each lane
    for a, l in enumerate(amb):
        cnt = int(acc[:l].sum())
        acc[l] = v[l] <= i - cnt
        if a >= 1 and (v[l] <= i - int(ndef[l])) != (v[l] <= i - int(ndef[l]) - a):
            led.events[("ambiguous_depends", where)] += 1
    return acc


def stream_ledger(key, pos0, n):
    """Walk k_fy_stream's loop for np.random.shuffle(arange(n)) from the state (key, pos0) -> Ledger (J: int64 [n], J[0] = 0)."""
    top = int(n) - 1
    R = raw_words(key, pos0, 2 * top + 40 * MT_N)
    led = Ledger()
    J = np.zeros(int(n), np.int64)
    state ={"q": 0, "prev": "start", "twist": 0}

    def words(count):
        nonlocal R
        while state["q"] + count > len(R):          # (acceptance is at least one half: this happens for unlucky streams only)
            R = raw_words(key, pos0, 2 * len(R))
        return R[state["q"]:state["q"] + count]

    def enter(path):
        led.handovers[(state["prev"], state["twist"], path)] += 1
        if led.paths and led.paths[-1][0] == path and not state["twist"]:
            led.paths[-1][1] += 1
        else:
            if state["twist"]:
                led.paths.append(["TWIST", 1])
            led.paths.append([path, 1])
        state["prev"], state["twist"] = path, 0

    def store(acc, v, i):
        """J[i - (accepted before)] = draw for every accepted draw; returns the number accepted"""
        hit = np.flatnonzero(acc)
        J[i - np.arange(len(hit))] = v[hit]
        return len(hit)

    def one_pass(c, i, mask, where):
        w = np.zeros(64, np.int64)
        w[:c] = words(c)
        v = w & mask
        got = store(_resolve_pass(v, c, i, 64, led, where), v, i)
        state["q"] += c
        return got

    idx = min(int(pos0), MT_N)
    i = top
    while i >= 1:
        assert (min(int(pos0), MT_N) + state["q"]) % MT_N == idx % MT_N
        if idx >= MT_N:
            idx = 0
            state["twist"] = 1
            mask = fy_mask(i)
            low = (mask >> 1) + 1
            margin = (i - MT_N) - max(FY_TAIL, low)
            if margin in (0, -1) and i >= FY_TAIL:
                led.events[("fast_guard_equal" if margin == 0 else "fast_guard_missed_by_one", low)] += 1
            if i - MT_N >= FY_TAIL and i - MT_N >= low:
                enter("fast")
                # The ten passes of the block in one sweep (word 64 k + lane is draw `lane` of pass k, so the flat order is the
                # stream's): thresholds of the block's first step; an ambiguous draw of pass k at lane l is tested against
                # i_k - (accepted below l in pass k) with i_k = i0 - (accepted in the passes before) -- i0 - (accepted before it
                # in the block), the same number.
                v = words(MT_N) & mask
                i0 = i
                definite = v <= i0 - MT_N
                acc = definite.copy()
                amb = np.flatnonzero(~definite & (v <= i0))
                seen = collections.Counter()     # pass -> ambiguous draws so far
                for l in amb:
                    k = int(l) // 64
                    acc[l] = v[l] <= i0 - int(acc[:l].sum())
                    a, seen[k] = seen[k], seen[k] + 1
                    if a == 1:
                        led.events[("two_ambiguous", "fast")] += 1
                    if a >= 1:
                        base = i0 - int(acc[:64 * k].sum()) - int(definite[64 * k:l].sum())      # against the definite draws alone
                        if (v[l] <= base) != (v[l] <= base - a):
                            led.events[("ambiguous_depends", "fast")] += 1
                i -= store(acc, v, i)
                state["q"] += MT_N
                idx = MT_N
                continue
            go = True
            for k in range(10):
                mk = fy_mask(i)
                lo = (mk >> 1) + 1
                if go and i >= FY_TAIL and i - 64 - lo in (0, -1):
                    led.events[("pass_guard_equal" if i - 64 == lo else "pass_guard_missed_by_one", "reg")] += 1
                go = go and i >= FY_TAIL and i - 64 >= lo
                if go:
                    c = MT_N - 576 if k == 9 else 64
                    enter("reg")
                    if k == 9:
                        led.events["ragged_tenth_register_pass"] += 1
                    i -= one_pass(c, i, mk, "pass")
                    idx += c
            continue
        mask = fy_mask(i)
        low = (mask >> 1) + 1
        if i >= FY_TAIL and i - 64 - low in (0, -1) and not state["twist"]:
            led.events[("pass_guard_equal" if i - 64 == low else "pass_guard_missed_by_one", "lds")] += 1
        if i < FY_TAIL or i - 64 < low:
            path = "serial_tail" if i < FY_TAIL else "serial_boundary"
            stop = 1 if i < FY_TAIL else low
            enter(path)
            w = words(MT_N - idx)
            used = 0
            while i >= stop and idx < MT_N:
                v = int(w[used]) & fy_mask(i)
                used += 1
                idx += 1
                if v <= i:
                    J[i] = v
                    i -= 1
            state["q"] += used
            if i >= stop:
                led.events[path + "_cut_by_block_end"] += 1
            continue
        c = min(64, MT_N - idx)
        enter("lds")
        if c < 64:
            led.events["ragged_lds_pass"] += 1
        i -= one_pass(c, i, mask, "pass")
        idx += c
    if top >= 1:
        led.handovers[(state["prev"], state["twist"], "end")] += 1
    if idx == MT_N:
        led.events["ends_on_block_end"] += 1
    led.J, led.draws, led.final_idx = J, state["q"], idx
    return led


_LEDGERS = {}


def ledger_of(case):
    """The ledger of a stream case, computed once per session."""
    if case not in _LEDGERS:
        kid, n, pos0 = case
        _LEDGERS[case] = stream_ledger(key_of(kid), pos0, n)
    return _LEDGERS[case]


# ---- the swaps ------------------------------------------------------------------------------------------------------------------
def swap_loop(J):
    """x = arange(n); for i = n-1 .. 1: swap(x[i], x[J[i]]) -- Fisher-Yates as numpy runs it, on given targets."""
    x = list(range(len(J)))
    Jl = [int(v) for v in J]
    for i in range(len(x) - 1, 0, -1):
        j = Jl[i]
        x[i], x[j] = x[j], x[i]
    return np.asarray(x, np.int64)


def resolve_rounds(n):
    """The doubling rounds the library runs: for (span = 1; span < n; span <<= 1)."""
    r, span = 0, 1
    while span < n:
        r, span = r + 1, span << 1
    return r


def resolve(J, max_rounds=None):
    """The parallel form of swap_loop as stage 3 of csrc/lgcn_shuffle.hip runs it (after tools/fy_parallel_prototype.py): sort the
    steps by (J[i], i); the parent of node p is the next step after p that targets p; pointer doubling, resolve_rounds(n) rounds
    (or max_rounds, to show what too few rounds do); position p holds the root of the first step that moves J[p] after step p."""
    J = np.asarray(J, np.int64)
    n = len(J)
    if n < 2:
        return np.arange(n, dtype=np.int64)
    comp = np.sort(J[1:] * (n + 1) + np.arange(1, n))

    def nxt(q, t):
        """smallest step i > t with J[i] == q, or -1"""
        pos = np.searchsorted(comp, q * (n + 1) + t, side='right')
        c = comp[np.minimum(pos, n - 2)]
        return np.where((pos < n - 1) & (c // (n + 1) == q), c % (n + 1), -1)

    nodes = np.arange(n)
    par = nxt(nodes, nodes)
    g = np.where(par >= 0, par, nodes)
    rounds = resolve_rounds(n) if max_rounds is None else min(resolve_rounds(n), max_rounds)
    for _ in range(rounds):
        g = g[g]
    q = J.copy()
    q[0] = 0
    first = nxt(q, nodes)
    return np.where(first >= 0, g[np.maximum(first, 0)], q).astype(np.int64)


def chain_depth(J):
    """The longest parent chain of the resolution (hops from a node to its root)."""
    J = np.asarray(J, np.int64)
    n = len(J)
    depth = np.zeros(n, np.int64)
    nxt_of = {}
    par = np.full(n, -1, np.int64)
    for i in range(n - 1, 0, -1):
        par[i] = nxt_of.get(i, -1)               # the smallest step > i that targets i: every later step is already entered
        nxt_of[int(J[i])] = i
    if n:
        par[0] = nxt_of.get(0, -1)
    for p in range(n - 1, -1, -1):               # parents have larger indices
        if par[p] >= 0:
            depth[p] = depth[par[p]] + 1
    return int(depth.max()) if n else 0


RESOLVE_NS = [2, 3, 255, 256, 257, 511, 512, 513, 4096, 4097, 65536, 65537, 180, 181, 361, 362]
SHIFTS = (2, 255, 256, 257)
RAMP_RS = (1, 4, 7, 10, 15)
UNIFORM_SEEDS = (11, 12, 13, 14)


def family_names(n):
    """The J families at size n.  A ramp needs 2^r + 1 <= n - 1; a size too small for any takes the one ramp L = n - 1."""
    names = ["chain", "identity", "zero", "half"] + [f"shift{s}" for s in SHIFTS]
    ramps = [f"ramp{(1 << r) + o}" for r in RAMP_RS if (1 << r) + 1 <= n - 1 for o in (-1, 0, 1)]
    names += ramps or [f"ramp{n - 1}"]
    return names + [f"uniform{s}" for s in UNIFORM_SEEDS]


def family_J(name, n):
    """uint32 [n] with J[0] = 0 and J[i] <= i."""
    i = np.arange(n, dtype=np.int64)
    if name == "chain":
        J = i - 1
    elif name == "identity":
        J = i.copy()
    elif name == "zero":
        J = np.zeros(n, np.int64)
    elif name == "half":
        J = i // 2
    elif name.startswith("shift"):
        J = np.maximum(i - int(name[5:]), 0)
    elif name.startswith("ramp"):
        J = np.where(i <= int(name[4:]), i - 1, i)
    elif name.startswith("uniform"):
        rng = np.random.Generator(np.random.PCG64(int(name[7:])))
        J = rng.integers(0, i + 1)
    else:
        raise KeyError(name)
    J[0] = 0
    assert (J >= 0).all() and (J <= i).all()
    return np.ascontiguousarray(J, np.uint32)


_WANT = {}


def resolve_want(name, n):
    """swap_loop of a family, computed once per session."""
    if (name, n) not in _WANT:
        _WANT[(name, n)] = swap_loop(family_J(name, n))
    return _WANT[(name, n)]
