"""Shared by the lossless-JPEG encoder tests: the images of the edge cases, the padded tiles and their reference streams
(tests/ljpeg_ref.py), and hhsr_ljpeg_encode_host / hhsr_ljpeg_encode / hhsr_ljpeg_histogram called with every buffer inside
guard bands."""
import ctypes
from collections import namedtuple

import numpy as np

import ljpeg_cases
import ljpeg_ref as ref

GUARD8 = 0xA5
Encoded = namedtuple("Encoded", "out offsets tile_bytes length intact")
UINT64_MAX = (1 << 64) - 1


def image(kind, H, W, Nf, P, seed=0):
    """uint16 [H, W, Nf]."""
    rng = np.random.default_rng(seed)
    if kind == "noise":  # full range: every category, many FF bytes
        return rng.integers(0, 1 << P, (H, W, Nf)).astype(np.uint16)
    if kind == "flat":
        img = np.full((H, W, Nf), 1 << (P - 1), np.uint16)  # the initial prediction too: one category
        return img
    if kind == "alt":  # alternating 0 / 32768: SSSS 16
        img = np.zeros((H, W, Nf), np.uint16)
        img[:, ::2] = 32768
        return img
    if kind == "smooth":  # photograph-like: small differences, short codes
        y, x = np.mgrid[0:H, 0:W]
        base = ((y * 37 + x * 53) % (1 << P))[:, :, None] + np.arange(Nf) * 11
        return ((base + rng.integers(0, 6, (H, W, Nf))) % (1 << P)).astype(np.uint16)
    raise ValueError(kind)


def tiles_of(img, th, tw):
    """The padded tiles [n_tiles, th, tw, Nf] in row-major order: the edge replicated."""
    H, W, Nf = img.shape
    ny, nx = -(-H // th), -(-W // tw)
    p = np.pad(img, ((0, ny * th - H), (0, nx * tw - W), (0, 0)), mode="edge")
    return p.reshape(ny, th, nx, tw, Nf).transpose(0, 2, 1, 3, 4).reshape(ny * nx, th, tw, Nf)


def ref_counts(img, P, predictor, th, tw):
    """int64 [Nf, 17]: np.bincount of ljpeg_ref.categories over the padded tiles."""
    Nf = img.shape[2]
    counts = np.zeros((Nf, 17), np.int64)
    for t in tiles_of(img, th, tw):
        _, ssss = ref.categories(t.astype(np.int64), P, predictor)
        for c in range(Nf):
            counts[c] += np.bincount(ssss[:, :, c].reshape(-1), minlength=17)
    return counts


def huffman(counts17):
    """hhsr_ljpeg_huffman -> (bits [16], values [n])."""
    from handheld_super_resolution import _lib

    c = np.ascontiguousarray(counts17, np.uint64)
    bits, values, n = np.zeros(16, np.uint8), np.zeros(17, np.uint8), ctypes.c_int()
    _lib.call("hhsr_ljpeg_huffman", c.ctypes.data, bits.ctypes.data, values.ctypes.data, ctypes.byref(n))
    assert not values[n.value:].any()
    return bits.tolist(), values[:n.value].tolist()


def tables_for(img, P, predictor, th, tw):
    return [huffman(c) for c in ref_counts(img, P, predictor, th, tw)]


def pack_tables(tables):
    bits = np.zeros((len(tables), 16), np.uint8)
    values = np.zeros((len(tables), 17), np.uint8)
    for i, (b, v) in enumerate(tables):
        bits[i], values[i, :len(v)] = b, v
    return bits, values


def ref_streams(img, P, predictor, th, tw, tables):
    Nf = img.shape[2]
    return [ref.encode(t.astype(np.int64), P, predictor, tables=tables, comp_table=list(range(Nf))) for t in tiles_of(img, th, tw)]


def pitched(img, row_elems):
    """(flat uint16 buffer with guard bands, offset of the first sample): rows row_elems apart, GUARD between and around."""
    H, W, Nf = img.shape
    band = 64
    row = W * Nf if row_elems is None else row_elems
    buf = np.full(band + H * row + band, ljpeg_cases.GUARD, np.uint16)
    view = buf[band:band + H * row].reshape(H, row)
    view[:, :W * Nf] = img.reshape(H, W * Nf)
    return buf, band, row


def encode_host(img, P, predictor, th, tw, tables, capacity=None, row_elems=None, band=64):
    """hhsr_ljpeg_encode_host -> Encoded (out: the bytes [0, min(capacity, length)))."""
    from handheld_super_resolution import _lib

    H, W, Nf = img.shape
    n = (-(-H // th)) * (-(-W // tw))
    sb, mb = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.call("hhsr_ljpeg_encode_workspace", H, W, Nf, th, tw, ctypes.byref(sb), ctypes.byref(mb))
    cap = mb.value if capacity is None else capacity
    src, lead, row = pitched(img, row_elems)
    out = np.full(band + cap + band, GUARD8, np.uint8)
    offsets, tb, length = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32), np.zeros(1, np.uint64)
    bits, values = pack_tables(tables)
    _lib.call("hhsr_ljpeg_encode_host", src[lead:].ctypes.data, H, W, Nf, row, P, predictor, th, tw, bits.ctypes.data,
              values.ctypes.data, out[band:].ctypes.data, cap, offsets.ctypes.data, tb.ctypes.data, length.ctypes.data)
    intact = bool((out[:band] == GUARD8).all() and (out[band + cap:] == GUARD8).all())
    L = int(length[0])
    return Encoded(out[band:band + (cap if L == UINT64_MAX else min(cap, L))].copy(), offsets, tb, L, intact)


def encode_gpu(img, P, predictor, th, tw, tables, capacity=None, row_elems=None, band=64, stream=None, out_shift=0):
    """hhsr_ljpeg_encode on the current device -> Encoded.  out_shift: bytes the output pointer is moved off 4-byte alignment."""
    import torch

    from handheld_super_resolution import _lib

    H, W, Nf = img.shape
    n = (-(-H // th)) * (-(-W // tw))
    sb, mb = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.call("hhsr_ljpeg_encode_workspace", H, W, Nf, th, tw, ctypes.byref(sb), ctypes.byref(mb))
    cap = mb.value if capacity is None else capacity
    dev = torch.device("cuda", torch.cuda.current_device())
    src, lead, row = pitched(img, row_elems)
    bits, values = pack_tables(tables)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        d_src = torch.as_tensor(src.view(np.int16)).to(dev)
        band += out_shift
        d_out = torch.full((band + cap + 64,), GUARD8, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_tb = torch.zeros(n, dtype=torch.int32, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        d_scr = torch.zeros(sb.value // 8 + 1, dtype=torch.int64, device=dev)
        _lib.call("hhsr_ljpeg_encode", ctypes.c_void_p(d_src.data_ptr() + 2 * lead), H, W, Nf, row, P, predictor, th, tw,
                  bits.ctypes.data, values.ctypes.data, _lib.ptr(d_scr), d_scr.numel() * 8,
                  ctypes.c_void_p(d_out.data_ptr() + band), cap, _lib.ptr(d_off), _lib.ptr(d_tb), _lib.ptr(d_len), _lib.stream())
        out = d_out.cpu().numpy()
        offsets, tb = d_off.cpu().numpy().view(np.uint64), d_tb.cpu().numpy().view(np.uint32)
        L = int(d_len.cpu().numpy().view(np.uint64)[0])
    intact = bool((out[:band] == GUARD8).all() and (out[band + cap:] == GUARD8).all())
    return Encoded(out[band:band + (cap if L == UINT64_MAX else min(cap, L))].copy(), offsets, tb, L, intact)


def histogram_gpu(img, P, predictor, th, tw, row_elems=None):
    """hhsr_ljpeg_histogram -> (counts int64 [Nf, 17], status, guards intact?)."""
    import torch

    from handheld_super_resolution import _lib

    H, W, Nf = img.shape
    sb, mb = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.call("hhsr_ljpeg_encode_workspace", H, W, Nf, th, tw, ctypes.byref(sb), ctypes.byref(mb))
    dev = torch.device("cuda", torch.cuda.current_device())
    src, lead, row = pitched(img, row_elems)
    d_src = torch.as_tensor(src.view(np.int16)).to(dev)
    band = 8
    d_cnt = torch.full((band + Nf * 17 + band,), -3, dtype=torch.int64, device=dev)
    d_st = torch.full((1,), -7, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(sb.value // 8 + 1, dtype=torch.int64, device=dev)
    _lib.call("hhsr_ljpeg_histogram", ctypes.c_void_p(d_src.data_ptr() + 2 * lead), H, W, Nf, row, P, predictor, th, tw,
              ctypes.c_void_p(d_cnt.data_ptr() + 8 * band), _lib.ptr(d_st), _lib.ptr(d_scr), d_scr.numel() * 8, _lib.stream())
    c = d_cnt.cpu().numpy()
    intact = bool((c[:band] == -3).all() and (c[band + Nf * 17:] == -3).all())
    return c[band:band + Nf * 17].reshape(Nf, 17), int(d_st.item()), intact


def decode_tiles(data, offsets, tile_bytes, H, W, Nf, th, tw):
    """Every tile stream through hhsr_ljpeg_parse + hhsr_ljpeg_decode_host (seg_w = tile_w Nf) -> uint16 [H, W, Nf]."""
    nx = -(-W // tw)
    items = []
    for i in range(len(tile_bytes)):
        o = int(offsets[i])
        items.append((bytes(data[o:o + int(tile_bytes[i])]), 0, (i % nx) * tw * Nf, (i // nx) * th, tw * Nf, th))
    plan = ljpeg_cases.plan_from_streams(items, 1, H, W * Nf)
    got, status, intact = ljpeg_cases.decode_host(plan)
    assert intact and not status.any(), status
    return got[0].reshape(H, W, Nf)


def check_layout(enc, n_tiles):
    """Even offsets, streams one after the other, the pad byte counted by the offsets and not by tile_bytes."""
    assert int(enc.offsets[0]) == 0 and int(enc.offsets[n_tiles]) == enc.length
    for i in range(n_tiles):
        o, nb, nxt = int(enc.offsets[i]), int(enc.tile_bytes[i]), int(enc.offsets[i + 1])
        assert o % 2 == 0 and nxt == o + nb + (nb & 1), (i, o, nb, nxt)
