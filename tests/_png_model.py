"""The device PNG encoder (csrc/png.hip; include/upflow_hip.h, upf_png_encode) restated in numpy and Python integers: the same
filter, histogram, tree construction and tie-breaking, halving rule, flat-code choice, header and bit packing.  encode() gives the
exact bytes of the zlib stream the kernels write for one image.

The stream: 78 01, ONE final dynamic-Huffman deflate block whose every symbol is a literal (no matches), a big-endian Adler-32.
    block header   BFINAL=1, BTYPE=2, HLIT=0 (257 literal/length codes), HDIST=0 (one distance code), HCLEN=15 (19 entries);
                   the code-length code gives 4 bits to the symbols 0..15 and none to 16..18, so its canonical codes are the
                   symbols themselves; then 258 lengths of 4 bits each (257 literal/length, one distance code of length 1).
    the code       Huffman over the 256 byte counts and ONE end-of-block: the symbols with a count, sorted by (count, symbol), merged
                   with two queues (leaves, and internal nodes in the order they were made); on equal weights a leaf goes before
                   an internal node.  A deepest leaf beyond 15 bits: every non-zero count becomes (count + 1) >> 1, and again.
                   Against it the flat code: 9 bits for the two first symbols in (count, symbol) order over all 257, 8 for the
                   rest.  The flat code is taken when it costs strictly fewer bits over the true counts.
    bits           deflate packs from the least significant bit; Huffman codes go in most significant bit first."""
import zlib

import numpy as np

EOB = 256
NSYM = 257
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4                 # 1106
MAX_BITS = 15


def filtered(img):
    """img [H,W,C] uint8 / uint16 -> the H * (stride + 1) bytes flow_io.write_png compresses: filter type 2, then cur - above."""
    img = np.asarray(img)
    h = img.shape[0]
    rows = np.ascontiguousarray(img.astype('>u2') if img.dtype == np.uint16 else img).view(np.uint8).reshape(h, -1)
    up = rows.copy()
    up[1:] = rows[1:] - rows[:-1]
    return np.concatenate([np.full((h, 1), 2, dtype=np.uint8), up], axis=1).reshape(-1)


def cap_bytes(n):
    """the pitch of an image's slot: n + n / 8 + 1024, rounded up to 16"""
    return (n + n // 8 + 1024 + 15) // 16 * 16


def huffman_lengths(freq):
    """freq: NSYM counts -> (NSYM code lengths, 0 for a symbol without a count; the depth of the deepest leaf)"""
    order = sorted((s for s in range(NSYM) if freq[s] > 0), key=lambda s: (freq[s], s))
    m = len(order)
    lens = [0] * NSYM
    if m == 1:
        lens[order[0]] = 1
        return lens, 1
    lw = [freq[s] for s in order]
    iw, pl, pi = [], [0] * m, [0] * (m - 1)
    li = ii = 0
    for k in range(m - 1):
        w = 0
        for _ in range(2):
            if li < m and (ii >= k or lw[li] <= iw[ii]):
                w += lw[li]
                pl[li] = k
                li += 1
            else:
                w += iw[ii]
                pi[ii] = k
                ii += 1
        iw.append(w)
    depth = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        depth[k] = depth[pi[k]] + 1
    for i, s in enumerate(order):
        lens[s] = depth[pl[i]] + 1
    return lens, max(lens)


def code_lengths(hist):
    """hist: 256 byte counts -> (NSYM lengths, info); info: 'halvings', 'deepest' (of the Huffman code), 'flat' (taken),
    'huff_bits', 'flat_bits' (the data and the end-of-block over the true counts)"""
    true = [int(x) for x in hist] + [1]
    freq, halvings = list(true), 0
    while True:
        lens, deepest = huffman_lengths(freq)
        if deepest <= MAX_BITS:
            break
        freq = [(f + 1) >> 1 if f else 0 for f in freq]
        halvings += 1
    rare = sorted(range(NSYM), key=lambda s: (true[s], s))[:2]
    flat = [9 if s in rare else 8 for s in range(NSYM)]
    huff_bits = sum(f * l for f, l in zip(true, lens))
    flat_bits = sum(f * l for f, l in zip(true, flat))
    take_flat = flat_bits < huff_bits
    return (flat if take_flat else lens), dict(halvings=halvings, deepest=deepest, flat=take_flat, huff_bits=huff_bits, flat_bits=flat_bits)


def canonical_codes(lens):
    """deflate's canonical code of `lens`, each code bit-reversed (ready to be packed from the least significant bit)"""
    count = [0] * (MAX_BITS + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (MAX_BITS + 2), 0
    for b in range(1, MAX_BITS + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(0)
            continue
        c = nxt[l]
        nxt[l] += 1
        out.append(int(format(c, '0%db' % l)[::-1], 2))
    return out


def encode_stream(data, info=None):
    """data: the filtered bytes (uint8 array) -> the zlib stream, bytes"""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    lens, inf = code_lengths(np.bincount(data, minlength=256))
    if info is not None:
        info.update(inf)
    codes = canonical_codes(lens)
    head, pos = 0, 0

    def put(value, nbits):
        nonlocal head, pos
        head |= value << pos
        pos += nbits
    put(0x78, 8)
    put(0x01, 8)
    put(1, 1)                                                   # BFINAL
    put(2, 2)                                                   # BTYPE = dynamic
    put(0, 5)                                                   # HLIT: 257 codes
    put(0, 5)                                                   # HDIST: 1 code
    put(15, 4)                                                  # HCLEN: 19 entries
    for s in CLC_ORDER:
        put(4 if s < 16 else 0, 3)
    for l in list(lens) + [1]:
        put(int(format(l, '04b')[::-1], 2), 4)                  # code-length code: symbol l, code l, 4 bits, reversed
    assert pos == 16 + HEADER_BITS
    sym_len = np.array(lens[:256], dtype=np.int64)[data]
    sym_code = np.array(codes[:256], dtype=np.int64)[data]
    start = pos + np.concatenate([[0], np.cumsum(sym_len)[:-1]])
    total = pos + int(sym_len.sum()) + lens[EOB]
    nbytes = (total + 7) // 8
    bits = np.zeros(nbytes * 8, dtype=np.uint8)
    hb = np.frombuffer(head.to_bytes((pos + 7) // 8, 'little'), dtype=np.uint8)
    bits[:hb.size * 8] = np.unpackbits(hb, bitorder='little')
    for k in range(MAX_BITS):
        sel = sym_len > k
        bits[start[sel] + k] = (sym_code[sel] >> k) & 1
    e = total - lens[EOB]
    for k in range(lens[EOB]):
        bits[e + k] = (codes[EOB] >> k) & 1
    return np.packbits(bits, bitorder='little').tobytes() + (zlib.adler32(data.tobytes()) & 0xffffffff).to_bytes(4, 'big')


def encode(img, info=None):
    """img [H,W,C] uint8 / uint16 -> the zlib stream of its PNG, as upf_png_encode writes it"""
    return encode_stream(filtered(img), info)


# ---- the images both test files encode ----------------------------------------------------------------------------------------------
CHUNK = 4096                                                    # bytes of the filtered stream per workgroup (csrc/png.hip)


def smooth(h, w, c, dtype, seed=0):
    """a flow-like field: slow waves and a little noise, scaled into the range of `dtype`"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    top = np.iinfo(dtype).max
    planes = [np.sin(xx / (7.0 + 3 * k) + seed) * np.cos(yy / (11.0 + k)) * 0.02 + 0.5 + g.normal(0.0, 2.0 / top, (h, w)) for k in range(c)]
    return np.clip(np.stack(planes, axis=-1) * top, 0, top).astype(dtype)


def fibonacci_row():
    """[1,W,1] uint8 whose filtered stream (the filter type 2 in front) has 30 values with the counts 1, 1, 2, 3, 5, ... 832040"""
    counts = [1, 1]
    while len(counts) < 30:
        counts.append(counts[-1] + counts[-2])
    row = np.concatenate([np.full(n - (v == 2), v, dtype=np.uint8) for v, n in zip(range(2, 32), counts)])
    np.random.default_rng(7).shuffle(row)
    return row.reshape(1, -1, 1)


def cases():
    """-> {tag: image [H,W,C]}"""
    g = np.random.default_rng(11)
    out = {
        'smooth u16x3': smooth(24, 40, 3, np.uint16),
        'smooth u8x3': smooth(24, 40, 3, np.uint8),
        'u8x1': smooth(9, 31, 1, np.uint8, 1),
        'u8x2': smooth(9, 31, 2, np.uint8, 2),
        'u8x4': smooth(9, 31, 4, np.uint8, 3),
        'u16x1': smooth(6, 10, 1, np.uint16, 4),
        'one row': smooth(1, 50, 3, np.uint16, 5),
        'one column': smooth(50, 1, 3, np.uint8, 6),
        'one pixel': np.array([[[2]]], dtype=np.uint8),
        'row of 6 bytes': smooth(7, 5, 1, np.uint8, 7),          # stride + 1 = 6: no multiple of 4
        'all zero': np.zeros((12, 20, 3), dtype=np.uint16),
        # (enough bytes that the largest count stays below twice the smallest: the Huffman tree is then the balanced one)
        'uniform random': g.integers(0, 256, (250, 400, 1)).astype(np.uint8),
        'fibonacci': fibonacci_row(),
        'many chunks': smooth(37, 53, 3, np.uint16, 8),
    }
    for d in (-1, 0, 1):                                         # a filtered stream of one chunk, a byte less, a byte more
        out['chunk%+d' % d] = g.integers(0, 7, (1, CHUNK + d - 1, 1)).astype(np.uint8)
    return out
