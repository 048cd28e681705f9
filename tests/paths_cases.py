"""What test_paths.py and test_paths_host.py share: the plain-loop numpy oracle of dff_path_states' definitions (include/dff.h)
and the seeded series the tests run on.  No GPU, no torch."""
import numpy as np

LO, HI = 0.2, 0.9
M = np.float32(0.5)                                                 # between the cores
KEYS_FRAME = ("prev", "next", "t_prev", "t_next", "cls")
KEYS_PATH = ("exit", "entry", "direction")


def frame_codes(cv, lo, hi):
    """-2 non-finite, 0 core A (cv <= lo), 1 core B (cv >= hi), -1 between: on the float32 values the kernel sees"""
    cv = np.asarray(cv, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    code = np.full(len(cv), -1, np.int64)
    code[cv <= lo] = 0
    code[cv >= hi] = 1
    code[~np.isfinite(cv)] = -2
    return code


def _tables(code, lengths, prev, nxt, t_prev, t_next):
    """the classes and the path table from the codes and the two visits of every frame"""
    n = len(code)
    cls = np.full(n, -1, np.int8)
    for t in range(n):
        if code[t] >= 0:
            cls[t] = code[t]
        elif code[t] == -1 and prev[t] >= 0 and nxt[t] >= 0:
            cls[t] = {(0, 1): 2, (1, 0): 3, (0, 0): 4, (1, 1): 5}[(int(prev[t]), int(nxt[t]))]
    exit_, entry, direction = [], [], []
    o = 0
    for ln in lengths:
        for e in range(o + 1, o + ln):                              # not the trajectory's first frame
            if code[e] >= 0 and prev[e - 1] >= 0 and prev[e - 1] != code[e]:
                exit_.append(t_prev[e - 1])
                entry.append(e)
                direction.append(code[e])
        o += ln
    return {"prev": prev, "next": nxt, "t_prev": t_prev, "t_next": t_next, "cls": cls, "exit": np.asarray(exit_, np.int64),
            "entry": np.asarray(entry, np.int64), "direction": np.asarray(direction, np.int8)}


def _lengths(code, lengths):
    lengths = [len(code)] if lengths is None else [int(v) for v in lengths]
    assert sum(lengths) == len(code) and min(lengths, default=0) >= 0
    return lengths


def path_states_by_walking(cv, lo, hi, lengths=None):
    """The definitions to the letter: from every frame, walk back and walk forward over the frames between the cores.  Quadratic
    in the length of an excursion: for short series; path_states_oracle gives the same in one pass per direction."""
    code = frame_codes(cv, lo, hi)
    n = len(code)
    lengths = _lengths(code, lengths)
    prev, nxt = np.full(n, -1, np.int8), np.full(n, -1, np.int8)
    t_prev, t_next = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    o = 0
    for ln in lengths:
        for t in range(o, o + ln):
            s = t
            while s >= o and code[s] == -1:                         # walk back, t included, over the frames between the cores
                s -= 1
            if s >= o and code[s] >= 0:
                prev[t], t_prev[t] = code[s], s
            s = t
            while s < o + ln and code[s] == -1:
                s += 1
            if s < o + ln and code[s] >= 0:
                nxt[t], t_next[t] = code[s], s
        o += ln
    return _tables(code, lengths, prev, nxt, t_prev, t_next)


def path_states_oracle(cv, lo, hi, lengths=None):
    """The oracle of dff_path_states, plain loops: per trajectory one pass forwards that remembers the last visit (a non-finite
    frame forgets it) and one backwards that remembers the next -> a dict of prev, next, cls int8 (n,), t_prev, t_next int64 (n,)
    and the path table exit, entry int64, direction int8 in ascending entry."""
    code = frame_codes(cv, lo, hi)
    n = len(code)
    lengths = _lengths(code, lengths)
    prev, nxt = np.full(n, -1, np.int8), np.full(n, -1, np.int8)
    t_prev, t_next = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    o = 0
    for ln in lengths:
        for out, t_out, frames in ((prev, t_prev, range(o, o + ln)), (nxt, t_next, range(o + ln - 1, o - 1, -1))):
            state, at = -1, -1
            for t in frames:
                if code[t] == -2:
                    state, at = -1, -1
                elif code[t] >= 0:
                    state, at = code[t], t
                out[t], t_out[t] = state, at
        o += ln
    return _tables(code, lengths, prev, nxt, t_prev, t_next)


def cv_series(n, seed, step=0.08):
    """a slow walk folded into 0 .. 1 with stretches in both cores and between them, exact threshold values, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    cv = np.abs(((0.55 + np.cumsum(rng.standard_normal(n)) * step) % 2.0) - 1.0).astype(np.float32)
    k = max(n // 60, 1)
    for val in (np.float32(LO), np.float32(HI), np.nextafter(np.float32(LO), np.float32(1)), np.nextafter(np.float32(HI), np.float32(0)),
                np.nan, np.inf, -np.inf):
        cv[rng.integers(0, n, k)] = val
    return cv


def ragged(n, n_traj, seed):
    """n_traj unequal lengths summing to n, one of them 0 and one of them 1"""
    lengths = np.random.default_rng(seed).integers(2, n // n_traj + 1, n_traj)
    lengths[3], lengths[5] = 0, 1
    lengths[-1] += n - lengths.sum()                                # the rest goes to the last one
    assert len(lengths) == n_traj and lengths.sum() == n and lengths.min() == 0
    return lengths.tolist()


CARRY_STRETCH = slice(520000, 526336)                              # the undetermined stretch of carry_case("one")


def carry_case(name):
    """Series of more than 256 x 2048 = 524 288 frames in one launch -> (cv, lengths).  The carry scan's one workgroup takes the
    blocks of a launch 256 at a time, so only such a launch makes it run a second chunk.
    one        257 x 2048 + 1 frames (258 blocks), one trajectory.  Frames 520 000 .. 526 335 lie between the cores, with core A
               on the frame before and core B on the one after (the lone frame of block 257): the stretch covers all of blocks
               255 and 256, on both sides of the chunk's edge, so its prev arrives only through the forward carry across the
               chunks, its next only through the reverse carry, and the path it ends is written from the second chunk.
    periodic   514 equal trajectories of 1025 frames: the periodic path above 256 blocks.
    groups     64 unequal trajectories of 8200 + i frames (one launch group of 258 blocks), then six short ones in a second
               group: the count of runs / paths goes into the second launch after a two-chunk carry."""
    if name == "one":
        cv = cv_series(257 * 2048 + 1, 1234, 0.3)
        cv[CARRY_STRETCH.start - 1], cv[CARRY_STRETCH], cv[CARRY_STRETCH.stop] = 0.0, M, 1.0
        return cv, [len(cv)]
    lengths = {"periodic": [1025] * 514, "groups": [8200 + i for i in range(64)] + [300, 1, 700, 2047, 5, 900]}[name]
    return cv_series(sum(lengths), 4321, 0.3), lengths


def reverse_within(a, lengths):
    """every trajectory of the series a reversed in place (the order of the trajectories stays)"""
    a = np.asarray(a)
    out, o = a.copy(), 0
    for ln in lengths:
        out[o:o + ln] = a[o:o + ln][::-1]
        o += ln
    return out


def reversed_times(t, lengths):
    """frame indices t (n,) of a series (-1: none), mapped to where those frames lie after reverse_within, in reversed order"""
    t = np.asarray(t, np.int64)
    out, o = t.copy(), 0
    for ln in lengths:
        seg = t[o:o + ln][::-1]
        out[o:o + ln] = np.where(seg >= 0, 2 * o + ln - 1 - seg, -1)
        o += ln
    return out
