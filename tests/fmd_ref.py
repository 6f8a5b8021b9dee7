"""Plain Python decoder of fermi's .fmd format (rld0.c:107-151, 207-244), for the tests of rb2_hip_load_fmd.

A block's runs are found the way the reference's reader finds them (rld_dec, rld0.h:79-116): by decoding until only zero padding is
left in the block -- NOT by the counts in the next header, so that comparing the two is a check of both.  Small files only."""
import gzip
import os
import struct

import numpy as np

GOLDEN_FMD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fmd")
FIXTURES = ["kat6", "rand300", "cov3000", "longA"]
HDR_WORDS = (2, 4, 7)
BLK = 8                                   # words per block
CHUNK = 1 << 23                           # words per chunk: its last block has a payload one word shorter (rld0.h:75)


def parse(img):
    """header fields and the stream as uint64 words"""
    img = bytes(img)
    assert img[:4] == b"RLD\3", "magic"
    ab, = struct.unpack_from("<I", img, 4)
    assert ab >> 16 == 6 and ab & 0xffff == 3, "asize / sbits"
    _, n_bytes, n_frames = struct.unpack_from("<3Q", img, 8)
    mcnt = list(struct.unpack_from("<6Q", img, 32))
    assert n_bytes % 8 == 0 and len(img) == 80 + n_bytes + 56 * n_frames, "file size"
    words = np.frombuffer(img, dtype="<u8", count=n_bytes // 8, offset=80)
    return {"n_bytes": n_bytes, "n_frames": n_frames, "mcnt": mcnt, "words": words}


def header(words, o):
    """(type, [total, $, A, C, G, T, N]) of the header at word o; the type bits are masked out of the count field they sit in"""
    w = [int(x) for x in words[o:o + 7]]
    t = w[0] >> 62
    assert t < 3, "header type"
    if t == 0:
        f = [(w[i // 4] >> (16 * (i % 4))) & 0x3fff for i in range(7)]
    elif t == 1:
        f = [(w[i // 2] >> (32 * (i % 2))) & 0x3fffffff for i in range(7)]
    else:
        f = [w[0] & ((1 << 62) - 1)] + w[1:7]
    return t, f


def block_runs(words, j):
    """the runs (symbol, length) of block j, decoded until the rest of the payload is zero padding"""
    o = j * BLK
    t, _ = header(words, o)
    end = BLK - 1 if (o + BLK) % CHUNK == 0 else BLK          # payload words [HDR_WORDS[t], end)
    bits = 0
    for k in range(HDR_WORDS[t], end):
        bits = bits << 64 | int(words[o + k])
    n = 64 * (end - HDR_WORDS[t])
    runs, p = [], 0
    while p < n and bits & ((1 << (n - p)) - 1):
        z = 0
        while not (bits >> (n - 1 - p - z)) & 1:
            z += 1
        y = ((bits >> (n - p - 2 * z - 1)) & ((1 << (z + 1)) - 1)) - 1     # gamma code of y + 1
        p += 2 * z + 1
        assert p + y + 3 <= n, "a code straddles the block"
        low = (bits >> (n - p - y)) & ((1 << y) - 1)
        p += y
        c = (bits >> (n - p - 3)) & 7
        p += 3
        assert c <= 5, "symbol code"
        runs.append((c, 1 << y | low))
    return runs


def decode(img):
    """{'mcnt', 'blocks': [(type, header fields, runs)], 'last': header fields of the closing header, 'runs': all runs, merged}"""
    h = parse(img)
    words = h["words"]
    nb, tail = divmod(len(words), BLK)
    t_last, f_last = header(words, nb * BLK)
    assert tail == HDR_WORDS[t_last], "the stream must end with a header alone"
    blocks = []
    for j in range(nb):
        t, f = header(words, j * BLK)
        blocks.append((t, f, block_runs(words, j)))
    runs = []
    for _, _, rs in blocks:
        for c, l in rs:
            if runs and runs[-1][0] == c:
                runs[-1][1] += l
            else:
                runs.append([c, l])
    return {"mcnt": h["mcnt"], "blocks": blocks, "last": f_last, "runs": runs, "words": words}


def symbols(runs):
    if not runs:
        return np.zeros(0, np.uint8)
    r = np.asarray(runs, dtype=np.int64)
    return np.repeat(r[:, 0].astype(np.uint8), r[:, 1])


def ropes(img):
    """the six ropes as nt6 arrays: the symbol stream cut at the boundaries the marginal counts give"""
    d = decode(img)
    s = symbols(d["runs"])
    cut = np.concatenate([[0], np.cumsum(d["mcnt"])])
    assert cut[-1] == len(s)
    return [s[cut[b]:cut[b + 1]] for b in range(6)]


def fixture(name):
    """(.fmd image as bytes, BWT as an nt6 array) of a fixture under tests/golden/fmd"""
    img = open(os.path.join(GOLDEN_FMD, name + ".fmd"), "rb").read()
    text = gzip.open(os.path.join(GOLDEN_FMD, name + ".bwt.gz"), "rb").read().replace(b"\n", b"")
    lut = np.full(256, 255, np.uint8)
    for i, ch in enumerate(b"$ACGTN"):
        lut[ch] = i
    bwt = lut[np.frombuffer(text, np.uint8)]
    assert (bwt != 255).all()
    return img, bwt
