"""cf_deflate / cf_crc32 (csrc/deflate.hip) against zlib, exactly: every stream, closed with the final block 03 00, must inflate under
zlib.decompress(stream, -15) to the bytes it was made from; it never exceeds cf_deflate_bound(n) nor touches a byte past it or past the
workspace; the same input gives the same bytes whatever the buffers held; the CRC equals zlib.crc32.  The size bars hold the match finder
and the Huffman coder to what the issue measured for zlib on the same bytes (comparators computed here with the stdlib)."""
import heapq
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
FINAL = b"\x03\x00"


def _lib():
    from cineflow import _lib as L
    return L.lib()


def _ch():
    return int(_lib().cf_deflate_chunk_bytes())


def _dev(data):
    """bytes / uint8 numpy -> uint8 device tensor (one spare byte, so that an empty input still has an address)"""
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    t = torch.empty(a.size + 1, dtype=torch.uint8, device="cuda")
    t[:a.size] = torch.from_numpy(a.copy())
    return t[:a.size]


def _deflate(src, fill=0xA5):
    """src: a contiguous device tensor.  Exact capacities, GUARD bytes of `fill` behind out and ws -> the stream (without the final block)"""
    h = _lib()
    n = src.numel() * src.element_size()
    cap, wsb = int(h.cf_deflate_bound(n)), int(h.cf_deflate_workspace_bytes(n))
    out = torch.full((cap + GUARD,), fill, dtype=torch.uint8, device="cuda")
    ws = torch.full((wsb + GUARD,), fill, dtype=torch.uint8, device="cuda")
    nb = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    rc = h.cf_deflate(src.data_ptr() or out.data_ptr(), n, out.data_ptr(), cap, ws.data_ptr(), wsb, nb.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, h.cf_last_error()
    k = int(nb.cpu())
    assert 0 <= k <= cap, (k, cap)
    assert bool((out[cap:] == fill).all()) and bool((ws[wsb:] == fill).all()), "a guard byte was written"
    if fill == 0xA5 and k < cap:
        assert bool((out[k:cap] == fill).all()), "bytes past the stream's end were written"
    return out[:k].cpu().numpy().tobytes()


def _crc(src):
    h = _lib()
    n = src.numel() * src.element_size()
    wsb = int(h.cf_crc32_workspace_bytes(n))
    ws = torch.full((wsb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    crc = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = h.cf_crc32(src.data_ptr() or ws.data_ptr(), n, ws.data_ptr(), wsb, crc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, h.cf_last_error()
    assert bool((ws[wsb:] == 0xA5).all()) and int(crc[1].cpu()) == 0x5A5A5A5A
    return int(crc[0].cpu()) & 0xFFFFFFFF


def _check(data, what):
    data = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    src = _dev(data)
    stream = _deflate(src)
    assert zlib.decompress(stream + FINAL, -15) == data, what
    assert _crc(src) == zlib.crc32(data), what
    return stream


def _lengths():
    CH = _ch()
    return [0, 1, 2, 3, 4, 257, 258, 259, 260, CH - 1, CH, CH + 1, 2 * CH + 7, 5 * CH + 1]


def _content(kind, n):
    rs = np.random.RandomState(n % 1000 + 11)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "random":
        return rs.randint(0, 256, n, dtype=np.uint8)
    if kind == "skewed":
        return rs.choice(np.array([65, 67, 71, 84], np.uint8), size=n, p=[0.7, 0.2, 0.08, 0.02])
    if kind == "mod251":
        return (np.arange(n) % 251).astype(np.uint8)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["zeros", "random", "skewed", "mod251"])
def test_every_length_inflates_to_its_source(kind):
    CH = _ch()
    for n in _lengths():
        stream = _check(_content(kind, n), (kind, n))
        chunks = -(-n // CH)
        assert len(stream) <= n + 5 * chunks
        if kind == "random" and n >= 260:
            assert len(stream) == n + 5 * chunks           # no match, flat histogram: every chunk is a stored block
        if kind == "zeros" and n >= 260:
            assert len(stream) <= 64 * chunks              # 258-byte matches at distance 1 under one distance code


@pytest.mark.parametrize("period", [1, 2, 3, 4, 8, 224, 896, -1])
def test_exact_periods(period):
    CH = _ch()
    period = CH - 1 if period < 0 else period
    n = 2 * CH + 7
    base = np.random.RandomState(period).randint(0, 256, period, dtype=np.uint8)
    data = np.tile(base, n // period + 1)[:n]
    stream = _check(data, period)
    if period in (1, 2, 4, 8):
        assert len(stream) < 400              # the fixed distances: 128 matches of 258 bytes per chunk under one or two codes of 1-2 bits
    elif period <= 896:
        assert len(stream) < 0.1 * n          # the hash finds an earlier period (3 included: it is not among the fixed distances)


def _huffman_depth(counts):
    heap = [(c, 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def _huffman_cost(counts):
    heap, cost = [c for c in counts if c], 0
    heapq.heapify(heap)
    while len(heap) > 1:
        a = heapq.heappop(heap) + heapq.heappop(heap)
        cost += a
        heapq.heappush(heap, a)
    return cost


def _code_lengths(freq, max_bits):
    h = _lib()
    f = torch.tensor(freq, dtype=torch.int32, device="cuda")
    lens = torch.full((len(freq) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = h.cf_huffman_code_lengths(f.data_ptr(), len(freq), max_bits, lens.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, h.cf_last_error()
    assert bool((lens[len(freq):] == 0xA5).all())
    return lens[:len(freq)].cpu().numpy().astype(int)


@pytest.mark.parametrize("max_bits, n_fib", [(15, 22), (15, 30), (7, 12), (7, 19)])
def test_code_length_limit_on_fibonacci_weights(max_bits, n_fib):
    """The limiter alone, on a histogram that needs it whatever a match finder does: Fibonacci weights make the unrestricted tree
    n - 1 deep.  The code must stay complete (Kraft sum exactly 1: inflate refuses anything else), within the limit, and monotone."""
    fib = [1, 1]
    while len(fib) < n_fib:
        fib.append(fib[-1] + fib[-2])
    assert _huffman_depth(fib) == n_fib - 1 > max_bits
    rs = np.random.RandomState(n_fib)
    freq = np.zeros(n_fib + 9, dtype=np.int64)
    where = rs.permutation(len(freq))[:n_fib]
    freq[where] = fib                                     # unused symbols in between
    lens = _code_lengths(freq.tolist(), max_bits)
    assert ((lens > 0) == (freq > 0)).all() and lens.max() == max_bits
    assert sum(2 ** (max_bits - int(l)) for l in lens if l) == 2 ** max_bits
    order = np.argsort(freq[where])
    assert (np.diff(lens[where][order]) <= 0).all()          # heavier never longer


def test_code_lengths_are_huffmans_when_no_limit_acts():
    rs = np.random.RandomState(0)
    for n in (2, 3, 19, 30, 286):
        freq = rs.randint(40, 5000, n).astype(np.int64) * (rs.rand(n) > 0.2)         # weights within two decades: a shallow tree
        freq[:2] += 1
        assert _huffman_depth([f for f in freq if f]) <= 15
        lens = _code_lengths(freq.tolist(), 15)
        assert ((lens > 0) == (freq > 0)).all()
        assert (lens * freq).sum() == _huffman_cost(freq.tolist()), n          # optimal: the cost of any Huffman tree
        assert sum(2.0 ** -int(l) for l in lens if l) == 1.0
    # one used symbol, and none: two codes of one bit, as zlib writes them
    assert _code_lengths([0, 0, 7, 0], 15).tolist() == [1, 0, 1, 0]
    assert _code_lengths([0, 0, 0, 0], 15).tolist() == [1, 1, 0, 0]


def _de_bruijn_pairs(k):
    """an order-2 de Bruijn sequence over k symbols (Lyndon words): every ordered pair of symbols occurs once in its k * k entries"""
    a, seq = [0] * 4, []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def test_chunk_in_which_the_15_bit_limit_acts_inflates():
    """A chunk whose literal/length tree is 16 deep without the limit, compressed and inflated end to end.  Even bytes: 18 symbols with
    the counts 1, 2, 3, 5, ... 4181 (the end-of-block symbol is the other 1), shuffled.  Odd bytes: 128 other symbols in de Bruijn order,
    so no pair of neighbouring odd bytes occurs twice, no 4-byte string occurs twice, no match exists, and the histogram the chunk's coder
    sees is exactly the byte counts below: the test asserts both conditions itself."""
    CH = _ch()
    counts = [1, 2]
    while 2 * (sum(counts) + counts[-1] + counts[-2]) <= CH:
        counts.append(counts[-1] + counts[-2])
    steep = np.concatenate([np.full(c, 3 + 5 * s, np.uint8) for s, c in enumerate(counts)])
    np.random.RandomState(7).shuffle(steep)
    data = np.empty(2 * len(steep), np.uint8)
    data[0::2] = steep
    data[1::2] = np.array(_de_bruijn_pairs(128), np.uint8)[:len(steep)] + 128
    assert len({data[i:i + 4].tobytes() for i in range(len(data) - 3)}) == len(data) - 3, "a 4-byte string repeats: matches would change the histogram"
    hist = np.bincount(data)
    assert _huffman_depth([int(c) for c in hist if c] + [1]) > 15, "the fixture must need more than 15 bits without the limit"
    stream = _check(data, "steep literal-only chunk")
    assert stream[0] & 7 == 4 and len(stream) < len(data)          # one dynamic block (6 bits of entropy per byte)


def test_chunk_of_fibonacci_byte_counts_inflates():
    """The issue's fixture.  Its own counts make a tree 20 deep; what the ll alphabet of the chunk sees is flatter (the end-of-block symbol
    joins the two counts of 1, and matches absorb the frequent bytes: tools/deflate_hostcheck prints 12-13 for it); the chunk in which
    the limit does act is the test above, and the limiter alone has test_code_length_limit_on_fibonacci_weights."""
    CH = _ch()
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    while sum(fib) > CH:
        fib.pop()
    assert _huffman_depth(fib) > 15, "the fixture must need more than 15 bits without the limit"
    data = np.concatenate([np.full(c, 40 + 7 * s, np.uint8) for s, c in enumerate(fib)])
    np.random.RandomState(1234).shuffle(data)
    stream = _check(data, "fibonacci")
    assert len(stream) < len(data) / 2        # entropy 2.6 bits per byte; a stored block would say the coder gave up


def test_degenerate_chunks():
    CH = _ch()
    _check(np.full(CH, 0x7F, np.uint8), "one distinct byte")
    _check(np.full(5, 0x7F, np.uint8), "one distinct byte, no match possible")
    _check(np.tile(np.array([3, 200], np.uint8), CH // 2), "two bytes alternating")
    _check(np.tile(np.array([3, 200], np.uint8), 3), "two bytes alternating, short")
    rs = np.random.RandomState(3)
    for tail in (1, 2):
        _check(np.concatenate([rs.randint(0, 4, CH, dtype=np.uint8), rs.randint(0, 256, tail, dtype=np.uint8)]), "last chunk of %d" % tail)
        _check(np.concatenate([np.zeros(2 * CH, np.uint8), np.full(tail, 9, np.uint8)]), "zeros, then a last chunk of %d" % tail)


def test_literal_only_dynamic_block():
    """No 4-byte string occurs twice, so no match exists and no distance code is used; the skewed histogram still makes the dynamic block
    smaller than the stored one (entropy below 5.2 bits per byte: at most 0.65 n + a header of under 100 bytes < n)."""
    p = 0.9 ** np.arange(48)
    for seed in range(200):
        data = np.random.RandomState(seed).choice(np.arange(48, 96).astype(np.uint8), size=400, p=p / p.sum())
        grams = {data[i:i + 4].tobytes() for i in range(len(data) - 3)}
        if len(grams) == len(data) - 3:
            break
    else:
        raise AssertionError("no seed without a repeated 4-gram")
    stream = _check(data, "literal only")
    assert len(stream) < len(data)
    assert stream[0] & 7 == 4                  # BFINAL 0, BTYPE 10: a dynamic block


def _image():
    z, y, x = np.meshgrid(np.arange(4), np.arange(128), np.arange(112), indexing="ij")
    img = (np.sin(y / 17.0) + np.cos(x / 23.0) + 0.1 * np.random.RandomState(0).randn(4, 128, 112)).astype(np.float32)
    img[:, :128 // 6, :] = 0
    img[:, :, :112 // 7] = 0
    return img


def _labels():
    y, x = np.meshgrid(np.arange(128), np.arange(112), indexing="ij")
    r = np.hypot(y - 64, x - 56)
    lab = np.zeros((128, 112), np.float32)
    for k, radius in enumerate((45, 30, 15)):
        lab[r < radius] = k + 1
    return np.ascontiguousarray(np.broadcast_to(lab, (4, 128, 112)))


def test_views_of_float32_float16_and_uint8_tensors():
    img = _image()
    for a in (img, img.astype(np.float16), (img * 40).astype(np.uint8), img[:, 1:, 3:].copy()):
        t = torch.from_numpy(a).cuda()
        assert zlib.decompress(_deflate(t) + FINAL, -15) == a.tobytes(), a.dtype
        assert _crc(t) == zlib.crc32(a.tobytes())
    # an unaligned start: a view one byte into a buffer
    raw = torch.from_numpy(np.frombuffer(img.tobytes(), np.uint8).copy()).cuda()
    for off in (1, 2, 3):
        v = raw[off:off + 70001]
        want = img.tobytes()[off:off + 70001]
        assert zlib.decompress(_deflate(v) + FINAL, -15) == want and _crc(v) == zlib.crc32(want), off


def test_same_bytes_on_every_run_whatever_the_buffers_held():
    from cineflow import ops
    CH = _ch()
    rs = np.random.RandomState(8)
    data = np.concatenate([np.frombuffer(_image().tobytes(), np.uint8), rs.randint(0, 256, CH + 3, dtype=np.uint8),
                           np.frombuffer(_labels().tobytes(), np.uint8)[:3 * CH + 11]])
    src = _dev(data)
    first = _deflate(src, fill=0xA5)
    second = _deflate(src, fill=0xFF)
    assert first == second
    out, nb = ops.deflate(src)                         # the package's wrapper, buffers from the allocator
    assert out[:int(nb.cpu())].cpu().numpy().tobytes() == first
    assert zlib.decompress(first + FINAL, -15) == data.tobytes()


def test_crc32_of_3_mb():
    data = np.random.RandomState(4).randint(0, 256, 3 * 1000 * 1000 + 17, dtype=np.uint8)
    assert _crc(_dev(data)) == zlib.crc32(data.tobytes())
    data[:] = 0
    assert _crc(_dev(data)) == zlib.crc32(data.tobytes())


def _rle_chunked(raw, CH):
    total = 0
    for i in range(0, len(raw), CH):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        total += len(c.compress(raw[i:i + CH]) + c.flush(zlib.Z_SYNC_FLUSH))
    return total


def test_sizes_against_zlib():
    CH = _ch()
    img, lab = _image().tobytes(), _labels().tobytes()
    rnd = np.random.RandomState(6).randint(0, 256, len(img), dtype=np.uint8).tobytes()
    got = {k: len(_check(v, k)) + len(FINAL) for k, v in (("image", img), ("labels", lab), ("random", rnd))}
    level1 = {k: len(zlib.compress(v, 1)) for k, v in (("image", img), ("labels", lab))}
    rle = _rle_chunked(lab, CH)
    print("device / zlib sizes: image %d / level-1 %d (%.4f), labels %d / chunked Z_RLE %d (%.4f) / level-1 %d, random %d of %d"
          % (got["image"], level1["image"], got["image"] / level1["image"], got["labels"], rle, got["labels"] / rle, level1["labels"], got["random"],
             len(rnd)))
    assert got["image"] <= 1.05 * level1["image"]                       # (a) dynamic Huffman + the previous element's runs: 0.994-1.000
    assert got["labels"] <= 0.5 * rle                                   # (b) the previous voxel AND the previous row
    assert got["random"] - len(FINAL) <= len(rnd) + 5 * -(-len(rnd) // CH)      # (c)


def test_package_functions_on_device_tensors():
    from cineflow import deflate
    img = _image()
    t = torch.from_numpy(img).cuda()
    assert zlib.decompress(deflate.deflate_raw(t), -15) == img.tobytes()
    assert deflate.crc32(t) == zlib.crc32(img.tobytes())
    assert deflate.deflate_raw(t[:0]) == FINAL and deflate.crc32(t[:0]) == 0
    p = deflate.pack(t.half())
    assert p.size == img.size * 2 and p.crc == zlib.crc32(img.astype(np.float16).tobytes())
