"""tests/_png_model.py, the Python statement of the device PNG encoder (csrc/png.hip), against zlib and the PNG reader: every
stream inflates to the filtered scan lines (zlib.decompress checks the Adler-32 too), the file write_png_stream makes of it reads
back to the image bit for bit, and the stream fits the slot.  No GPU: test_hip_png.py holds the kernels to this model."""
import zlib

import numpy as np
import pytest

import _png_model as pm
from upflow_pytorch_amd.utils import flow_io


@pytest.fixture(scope='module')
def encoded():
    out = {}
    for tag, img in pm.cases().items():
        info = {}
        out[tag] = (img, pm.encode(img, info), info)
    return out


def test_every_stream_inflates_reads_back_and_fits(encoded, tmp_path):
    for tag, (img, stream, info) in encoded.items():
        raw = pm.filtered(img)
        h, w, c = img.shape
        depth = 8 * img.dtype.itemsize
        assert raw.size == h * (w * c * depth // 8 + 1), tag
        assert stream[:2] == b'\x78\x01' and zlib.decompress(stream) == raw.tobytes(), tag
        assert len(stream) <= pm.cap_bytes(raw.size), tag
        # nine bits for a byte and for the end-of-block at the most, whichever code was taken
        assert len(stream) <= 2 + (pm.HEADER_BITS + 9 * (raw.size + 1) + 7) // 8 + 4, tag
        fn = str(tmp_path / 'x.png')
        flow_io.write_png_stream(fn, w, h, depth, c, stream)
        back = flow_io.read_png(fn)
        assert back.dtype == img.dtype and np.array_equal(back, img), tag
        flow_io.write_png_stream(fn, w, h, depth, c, np.frombuffer(stream, dtype=np.uint8))     # (as the saver hands it over)
        assert np.array_equal(flow_io.read_png(fn), img), tag


def test_the_cases_are_what_they_are_meant_to_be(encoded):
    shapes = {tag: img.shape for tag, (img, _, _) in encoded.items()}
    assert {s[2] for s in shapes.values()} == {1, 2, 3, 4}
    assert shapes['one row'][0] == 1 and shapes['one column'][1] == 1 and shapes['one pixel'] == (1, 1, 1)
    assert (shapes['row of 6 bytes'][1] * shapes['row of 6 bytes'][2] + 1) % 4 != 0
    for d in (-1, 0, 1):
        assert pm.filtered(encoded['chunk%+d' % d][0]).size == pm.CHUNK + d
    assert pm.filtered(encoded['many chunks'][0]).size > 2 * pm.CHUNK
    assert {img.dtype for img, _, _ in encoded.values()} == {np.dtype(np.uint8), np.dtype(np.uint16)}


def test_an_all_zero_image_has_two_byte_values_at_one_bit_each(encoded):
    img, stream, info = encoded['all zero']
    raw = pm.filtered(img)
    assert set(raw.tolist()) == {0, 2}
    lens, _ = pm.code_lengths(np.bincount(raw, minlength=256))
    assert lens[0] == 1 and sorted(l for l in lens if l) == [1, 2, 2]
    assert len(stream) == 2 + (pm.HEADER_BITS + int((raw == 0).sum()) + 2 * int((raw == 2).sum()) + 2 + 7) // 8 + 4
    # the degenerate alphabet, which a stream never has (it always holds a filter type and the end-of-block): one bit
    assert pm.huffman_lengths([0] * 5 + [9] + [0] * 251) == ([0] * 5 + [1] + [0] * 251, 1)


def test_uniform_random_bytes_take_the_flat_code_or_tie(encoded):
    img, stream, info = encoded['uniform random']
    n = pm.filtered(img).size
    assert info['flat'] or info['flat_bits'] == info['huff_bits']
    assert info['flat_bits'] <= 9 * (n + 1)
    assert len(stream) <= 2 + (pm.HEADER_BITS + 9 * (n + 1) + 7) // 8 + 4


def test_the_flat_code_is_complete_and_taken_when_halving_spoils_the_tree():
    lens, info = pm.code_lengths(np.full(256, 1000))
    assert sum(2.0 ** -l for l in lens) == 1.0 and sorted(set(lens)) == [8, 9]
    # a tree that halving flattens badly: the flat code wins and is taken
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    hist = np.array(fib + [fib[-1]] * 216, dtype=np.int64)
    lens, info = pm.code_lengths(hist)
    assert info['halvings'] > 0
    assert info['flat'] == (info['flat_bits'] < info['huff_bits'])
    assert sum(f * l for f, l in zip(list(hist) + [1], lens)) == min(info['flat_bits'], info['huff_bits'])


def test_fibonacci_counts_go_through_the_halving_rule_to_exactly_15_bits(encoded):
    img, stream, info = encoded['fibonacci']
    counts = np.bincount(pm.filtered(img), minlength=256)
    assert sorted(counts[counts > 0].tolist())[:6] == [1, 1, 2, 3, 5, 8] and int((counts > 0).sum()) == 30
    unlimited, deepest = pm.huffman_lengths([int(x) for x in counts] + [1])
    assert deepest > pm.MAX_BITS
    assert info['halvings'] >= 1 and info['deepest'] == pm.MAX_BITS and not info['flat']
    lens, _ = pm.code_lengths(counts)
    assert max(lens) == pm.MAX_BITS and sum(2.0 ** -l for l in lens if l) == 1.0


def test_the_smooth_16_bit_field_comes_out_shorter_than_its_scan_lines(encoded):
    img, stream, info = encoded['smooth u16x3']
    assert len(stream) < pm.filtered(img).size


def test_ties_are_broken_by_symbol_and_a_leaf_goes_before_a_node():
    # four equal counts and the end-of-block: (EOB 1), then 10, 20, 30, 40 at 5 each.  Leaves sorted (1,256) (5,10) (5,20) (5,30)
    # (5,40): node0 = EOB + 10 (6); node1 = 20 + 30 (10); node2 = 40 + node0 (11): the leaf 40 before node0; node3 = node1 + node2
    freq = [0] * 257
    for s in (10, 20, 30, 40):
        freq[s] = 5
    freq[256] = 1
    lens, deepest = pm.huffman_lengths(freq)
    assert (lens[10], lens[20], lens[30], lens[40], lens[256]) == (3, 2, 2, 2, 3) and deepest == 3
    codes = pm.canonical_codes(lens)
    # canonical: the 2-bit codes 00, 01, 10 in symbol order, then 110 (10) and 111 (EOB); stored bit-reversed
    assert (codes[20], codes[30], codes[40], codes[10], codes[256]) == (0b00, 0b10, 0b01, 0b011, 0b111)
