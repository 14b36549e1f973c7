"""The directed NAL units of tests/harness/nal_core_check.c, generated in Python from the kernels'
geometry: units are (nal_ref_idc, nal_unit_type, head bytes, payload bytes)."""
import numpy as np

FOLLOW = (0, 1, 2, 3, 4, 0xFF)
ALPHABET = np.array([0, 0, 0, 1, 2, 3, 4, 0xFF], np.uint8)
HEAD_MAX = 64


def _unit(buf, hn, ref_idc=2, typ=1):
    buf = bytes(buf)
    hn = min(hn, len(buf))
    return (ref_idc, typ, buf[:hn], buf[hn:])


def run_unit(end, r, v, hn):
    """A zero run of r bytes that ends at `end`, the follower v behind it, filler elsewhere."""
    b = bytearray(b"\x55" * (end + 3))
    b[end - r:end] = bytes(r)
    b[end] = v
    return _unit(b, hn)


def runs_around(T):
    """For m in 1..3, d in -3..+3, r in 1..7 and every follower: the run ends at m * T + d; all
    payload, and behind a 7-byte head."""
    return [run_unit(m * T + d, r, v, hn) for m in (1, 2, 3) for d in range(-3, 4) for r in range(1, 8) for v in FOLLOW for hn in (0, 7)]


def runs_across_junction():
    """The run split by the head / payload junction at every split point: s of its r zeros end the
    head, for heads of s .. s + 9 and 58 .. 64 bytes (a head holds at most 64, so the junction meets
    the tile boundary at 64 and no other)."""
    out = []
    for r in range(1, 8):
        for s in range(r + 1):
            for v in FOLLOW:
                for hn in [h for h in list(range(s, s + 10)) + list(range(58, HEAD_MAX + 1)) if h >= s]:
                    out.append(run_unit(hn - s + r, r, v, hn))
    return out


def sized_units(T, rng):
    """Units of 0, 1, T - 1, T, T + 1 bytes over the zero-heavy alphabet, with and without a head."""
    out = []
    for n in (0, 1, T - 1, T, T + 1):
        for rep in range(8):
            out.append(_unit(ALPHABET[rng.integers(0, 8, n)].tobytes(), 5 if rep & 1 else 0, 3, 5))
    return out


def zero_chunks(chunk):
    """A middle chunk of zeros, and two of them in a row: 0..3 zeros end the chunk before, every follower behind."""
    out = []
    for zc in (1, 2):
        for pre in range(4):
            for v in FOLLOW:
                b = bytearray(b"\x77" * ((zc + 2) * chunk))
                b[chunk - pre:(zc + 1) * chunk] = bytes(pre + zc * chunk)
                b[(zc + 1) * chunk] = v
                out.append(_unit(b, 3))
    return out


def units_in_a_row():
    """One unit ends in 00 00, the next begins with 00: no carry may cross units.  An empty unit among them."""
    out = []
    for v in FOLLOW:
        for hn in (0, 1, 2):
            out += [_unit(b"\x09\x09\x09\x09\x00\x00", hn, 3, 5), _unit(bytes([0, v, 0, 0]), hn, 3, 5), _unit(bytes([0, 0, v]), hn),
                    _unit(b"", 0), _unit(bytes([0, 0, v]), 0)]
    return out


def random_units(n, chunk, rng):
    """n units of 0 .. 3 chunks over the alphabet, the head a random 0 .. 64 bytes of each."""
    out = []
    for _ in range(n):
        k = rng.integers(0, 8)
        size = int(rng.integers(0, 8) if k == 0 else rng.integers(0, 130) if k < 4 else rng.integers(0, 3 * chunk + 1))
        out.append(_unit(ALPHABET[rng.integers(0, 8, size)].tobytes(), int(rng.integers(0, HEAD_MAX + 1)), int(rng.integers(0, 4)),
                         int(rng.integers(1, 6))))
    return out


def zero_word_cases(nmb):
    """(unit, bins, bit depth, the words wanted): bins for an excess (3 bins - 36 bd nmb - 32 bytes) of
    0, 1, 96, 97, a negative one and 40 words and one, at bit depths 8 and 10.  The unit (one, no
    escapes) is sized so that 3 divides the right side; it ends in zeros, behind which the words go."""
    out = []
    for bd in (8, 10):
        for excess, want in ((0, 0), (1, 1), (96, 1), (97, 2), (-50, 0), (96 * 40 + 1, 41)):
            for size in (30, 31, 32):
                rhs = excess + 36 * bd * nmb + 32 * (1 + size)
                if rhs % 3 == 0:
                    out.append((_unit(b"\x55" * (size - 2) + b"\x00\x00", 4), rhs // 3, bd, want))
                    break
    return out
