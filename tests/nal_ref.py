"""Annex B packaging restated from the standard, the reference of the NAL tests (it shares nothing
with csrc/jmh_nal.h).

7.3.1 / 7.4.1: within a NAL unit, an emulation_prevention_three_byte 0x03 is inserted wherever the
next RBSP byte is 0x00..0x03 and the two bytes written before it are 0x00 0x00 -- the bytes *written*,
so an inserted 0x03 ends the run.  B.1: each unit is preceded by a start code, here the four-byte
form.  7.4.2.10 / 9.3.4.6: cabac_zero_words 0x0000 are appended to the last slice's RBSP until
BinCountsInNALunits <= 32/3 * NumBytesInVclNALunits + RawMbBits * PicSizeInMbs / 32; as RBSP bytes
behind a non-zero byte each becomes 00 00 03.  NumBytesInVclNALunits counts header byte and
escapes, not start codes; RawMbBits = 256 * BitDepthY + 2 * 64 * BitDepthC for 4:2:0."""


import re

_EMULATION = re.compile(rb"\x00\x00(?=[\x00-\x03])")


def nal_unit_bytewise(nal_ref_idc, nal_unit_type, rbsp):
    """The rule as the standard words it, a byte at a time."""
    out = bytearray(b"\x00\x00\x00\x01")
    out.append((nal_ref_idc << 5) | nal_unit_type)
    for v in bytes(rbsp):
        if v <= 3 and len(out) >= 7 and out[-1] == 0 and out[-2] == 0:
            out.append(3)
        out.append(v)
    return bytes(out)


def nal_unit(nal_ref_idc, nal_unit_type, rbsp):
    """The same through a left-to-right, non-overlapping substitution: behind two zero bytes that a
    byte 0..3 follows goes the 0x03, and the search goes on behind it, so the run starts anew."""
    return b"\x00\x00\x00\x01" + bytes([(nal_ref_idc << 5) | nal_unit_type]) + _EMULATION.sub(b"\x00\x00\x03", bytes(rbsp))


def zero_words(nbins, nbytes_vcl, nmb, bit_depth=8):
    """The cabac_zero_words a picture of nmb macroblocks needs: the smallest z >= 0 with
    nbins <= 32/3 * (nbytes_vcl + 3 z) + RawMbBits * nmb / 32, in integers (times 3)."""
    if nbins <= 0:
        return 0
    bd = max(bit_depth, 8)
    raw_mb_bits = 256 * bd + 128 * bd
    z = 0
    while 3 * 32 * nbins > 32 * 32 * (nbytes_vcl + 3 * z) + 3 * raw_mb_bits * nmb:
        z += 1
    return z


def access_unit(units, nbins=0, nmb=0, bit_depth=8):
    """units: (nal_ref_idc, nal_unit_type, head bytes, payload bytes) each.  Returns (the access
    unit's bytes, [(offset, nbytes)] of every NAL unit, start code included; the zero words count
    towards the last unit)."""
    out, where = bytearray(), []
    for ref_idc, typ, head, payload in units:
        nal = nal_unit(ref_idc, typ, bytes(head) + bytes(payload))
        where.append((len(out), len(nal)))
        out += nal
    z = zero_words(nbins, len(out) - 4 * len(units), nmb, bit_depth)
    out += b"\x00\x00\x03" * z
    if z:
        where[-1] = (where[-1][0], where[-1][1] + 3 * z)
    return bytes(out), where


def zero_words_closed_form(nbins, nbytes_vcl, nmb, bit_depth=8):
    bd = max(bit_depth, 8)
    excess = 3 * nbins - 36 * bd * nmb - 32 * nbytes_vcl
    return (excess + 95) // 96 if nbins > 0 and excess > 0 else 0


def census(units, tile, chunk):
    """How often an escape's zero run (the zero bytes of the input right before the escaped byte)
    reaches back over a tile boundary, a chunk boundary, the head / payload junction, a whole chunk
    of zeros: what the directed inputs are for.  From the reference's rule alone: in a run of zeros
    that starts at a, the substitution above puts a 0x03 before a + 2, a + 4, ... up to the byte
    behind the run when that one is 0..3."""
    got = {"escapes": 0, "tile": 0, "chunk": 0, "junction": 0, "zero_chunk": 0}
    for _, _, head, payload in units:
        s = bytes(head) + bytes(payload)
        for m in re.finditer(rb"\x00{2,}", s):
            a, b = m.span()
            last = b if b < len(s) and s[b] <= 3 else b - 1
            for i in range(a + 2, last + 1, 2):
                got["escapes"] += 1
                got["tile"] += a // tile != i // tile
                got["chunk"] += a // chunk != i // chunk
                got["junction"] += a < len(head) <= i
                got["zero_chunk"] += (a + chunk - 1) // chunk + 1 <= i // chunk
    return got
