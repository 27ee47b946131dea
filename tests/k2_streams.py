"""Hand-built streams for the batch decoders' tests (K2j, K2r, K2t) and the check they share.

The builders are host only: a stream is the header plus tokens written one by one (ez.Encoder),
so that a test decides every token's form, length, distance and position.  _run decodes a batch
with one decoder forced and checks, per stream: status, size and bytes equal the oracle's
(orc.decompress with the slot as capacity) and the exact decoder's; every output byte outside
[out_off[s], out_off[s] + size) keeps its 0xA5 sentinel (slot slack and the bytes before out_off[0]
included; for a stream that ends in an error only the bytes outside its slot); the input view is
surrounded by 0xFF bytes; and the streams handed to the exact decoder (the workspace's first
words: the count, then the stream indices) are exactly the ones expected.  All comparisons are
exact equality."""

import numpy as np

import oracle as orc

HDR = b"\x80\x02eazy\x80\x10\x14"  # magic, reset to a 1 MiB window
HDR_1K = b"\x80\x02eazy\x80\x10\x0a"  # magic, reset to a 1 KiB window
LIT, CPY = 0x00, 0x80
SMALL_MAX = 96 << 10  # jchunk: 256-byte chunks up to this much input in the batch, 1 KiB above
META_MAGIC, META_VER, META_RESET, META_BREAK = 0 << 3, 1 << 3, 2 << 3, 3 << 3


# ---------------------------------------------------------------- stream builders (host only)


def _E():
    import eazy_amd as ez

    return ez.Encoder()


def rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def lit(body):
    return _E().tag(b"", LIT, len(body)) + body


def cpy(d, n):
    """A copy of n bytes from d back, as Encoder.Offset writes it (d < n: the 0xff long prefix)."""
    e = _E()
    return e.offset(e.tag(b"", CPY, n), d, n)


def cpy_long(d, n):
    """The long prefix with a distance that does not need it (Decoder.Offset takes it all the same)."""
    e = _E()
    return e.tag(b"", CPY, n) + b"\xff" + e.offset(b"", d, 0)


def meta(m, arg=b""):
    return _E().meta(b"", m, len(arg)) + arg


def lit_to(c, target, rng):
    """c plus literals so that the stream is target bytes long."""
    e = _E()
    for extra in range(4):
        c2 = c + lit(b"q") * extra
        for tl in (1, 2, 3, 5):
            n = target - len(c2) - tl
            if n >= 1 and len(e.tag(b"", LIT, n)) == tl:
                out = c2 + lit(rb(rng, n))
                assert len(out) == target
                return out
    raise AssertionError((len(c), target))


def _forms(rng):
    """(name, bytes of the form, header length, whether it needs a 70,000-byte literal before it)"""
    f = [
        ("lit_len0", lit(rb(rng, 50)), 1, False),
        ("lit_len1", lit(rb(rng, 200)), 2, False),
        ("lit_len2", lit(rb(rng, 1000)), 3, False),
        ("lit_len4", lit(rb(rng, 70000)), 5, False),
        ("cpy_plain", cpy(30, 20), 2, False),
        ("cpy_off1", cpy(320, 20), 3, False),
        ("cpy_off2", cpy(720, 20), 4, False),
        ("cpy_len1_off1", cpy(500, 200), 4, False),
        ("cpy_len2", cpy(510, 500), 4, False),
        ("cpy_off4", cpy(66044 + 20 + 100, 20), 6, True),
        ("cpy_len4_run", cpy(1, 70000), 7, False),
        ("cpy_long", cpy_long(40, 20), 3, False),
        ("zero_region", cpy(0, 64), 3, False),
        ("break", meta(META_BREAK), 2, False),
        ("ver", meta(META_VER, b"\x00"), 3, False),
        ("magic", meta(META_MAGIC, b"eazy"), 6, False),
    ]
    for n in (1, 15, 16, 17, 40):
        f.append((f"pad{n}", bytes(n), n, False))
    return f


# ---------------------------------------------------------------- the check

_ORC = {}


def _oracle(b, cap, limit=0):
    """(output, error) of the oracle's Reader on b with a buffer of cap bytes (error 2: the output
    does not fit) and BlockSizeLimit = limit; cached per (stream, cap, limit)."""
    key = (b, cap, limit)
    if key not in _ORC:
        if limit == 0:
            want, err, _ = orc.decompress(b, cap=cap)
        else:  # or_decompress's loop, with the limit set
            r = orc.Reader(b=b)
            r.set(limit, 1 << 16)
            want, err = b"", 0
            while True:
                got, err = r.read(1 << 16)
                if len(want) + len(got) > cap:
                    err = orc.ESHORTBUF
                    break
                want += got
                if err == orc.EBREAK:
                    continue
                if err == orc.EOF:
                    err = 0
                if err != 0 or not got:
                    break
        _ORC[key] = (want, err)
    return _ORC[key]


def _need(b, limit=0):
    """The oracle's output length of a stream (its partial output, for a stream with an error)."""
    return len(_oracle(b, max(1 << 20, 4 * len(b)), limit)[0])


def _slot(s, need):
    n = need + 1 + s % 5
    return n + 1 if n % 16 == 0 else n


def assert_valid(named, limit=0):
    """Every stream of [(name, bytes)] decodes without an error on the oracle."""
    for name, b in named:
        assert _oracle(b, max(1 << 20, 4 * len(b)), limit)[1] == 0, name


GUARD = 64  # bytes of 0xFF on both sides of the input view


def _run(cuda, ins, jc=None, slots=None, handed="auto", hints=None, lead=5, kind="j", last=None, max_len=None,
         block_size_limit=0, pad=0, ws_init=0):
    """Decode ins with the decoder `kind` forced ("j", "r", "t"; "": the library's choice) and check
    everything the module's docstring lists.
    jc: the chunk size a K2j batch must take (asserted from its input).  slots: {index: slot bytes}
    overriding the default (the oracle's length plus 1..5 bytes, never a multiple of 16).
    handed: the stream indices the decoder must hand over ("auto": the ones the oracle gives an error or
    that do not fit their slot; "all": every stream; None: not checked).  hints: f(in_bytes, out_bytes) -> kwargs.
    last: the decoder the batch must have taken (default: kind).  max_len: the hint (True: the largest slot).
    pad: bytes (0xFF) inside the input view before comp_off[0] and after comp_off[count]; the view
    itself lies between two guards of 64 bytes of 0xFF.
    ws_init: what the workspace holds when the call starts, a fill byte or a tensor to copy from (an
    earlier call's workspace).  The workspace lies between two guards (tests/dirty.py), which must be
    intact afterwards; the exact decoder alone must leave all of it as it was.
    Returns (the workspace as the forced decoder left it, streams it handed over, literals it deferred)."""
    import torch

    import eazy_amd as ez
    from dirty import guarded, guards_intact, k2_lists

    count = len(ins)
    total_in = sum(len(b) for b in ins)
    if kind == "j":
        assert (256 if total_in <= SMALL_MAX else 1024) == jc, (total_in, jc)
    lim = block_size_limit
    cap = [slots[s] if slots and s in slots else _slot(s, _need(b, lim)) for s, b in enumerate(ins)]
    coff = pad + np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    ooff = lead + np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
    assert ooff[0] % 16 == 5
    ff = b"\xff" * (GUARD + pad)
    whole = torch.from_numpy(np.frombuffer(ff + b"".join(ins) + ff, np.uint8).copy()).to(cuda)
    comp = whole[GUARD : len(whole) - GUARD]
    assert comp.numel() == total_in + 2 * pad
    d_coff = torch.from_numpy(coff).to(cuda)
    d_ooff = torch.from_numpy(ooff).to(cuda)
    kw = hints(int(coff[-1] - coff[0]), int(ooff[-1] - ooff[0])) if hints else {}
    if max_len is not None:
        kw["max_len"] = max(cap) if max_len is True else max_len
    res = []
    for exact in (False, True):
        out = torch.full((int(ooff[-1]) + 64,), 0xA5, dtype=torch.uint8, device=cuda)
        sz = torch.full((count,), -7, dtype=torch.int64, device=cuda)
        st = torch.full((count,), -7, dtype=torch.int32, device=cuda)
        ws_whole, ws = guarded(cuda, ez._lib().ez_decompress_workspace(count), ws_init)
        ws0 = ws.clone()
        ez.select_decompress_kernel("" if exact else kind)
        try:
            ez.decompress_batch(comp, d_coff, d_ooff, block_size_limit=lim, out=out, sizes=sz, status=st, workspace=ws,
                                exact_only=exact, **kw)
            torch.cuda.synchronize()
            took = ez.decompress_kernel_last()
        finally:
            ez.select_decompress_kernel("")
        guards_intact(ws_whole, "the exact decoder" if exact else "K2" + kind)
        if not exact:
            assert took == (kind if last is None else last), took
            left, fast = ws.clone(), took
        else:
            assert torch.equal(ws, ws0), "the exact decoder alone wrote the workspace"
        res.append((out.cpu().numpy(), sz.cpu().numpy(), st.cpu().numpy(), ws[: 4 * (count + 1)].cpu().numpy().view(np.uint32)))
    (out, sz, st, w), (xout, xsz, xst, _) = res
    bad = set()
    inside = np.zeros(len(out), bool)  # bytes a decoder may have changed
    for s, b in enumerate(ins):
        want, err = _oracle(b, cap[s], lim)
        o = int(ooff[s])
        assert st[s] == xst[s] and sz[s] == xsz[s], (s, st[s], xst[s], sz[s], xsz[s])
        assert 0 <= sz[s] <= cap[s], (s, sz[s])
        n = int(sz[s])
        # (K2r and K2t may have written part of a slot before they hand a stream with an error over)
        inside[o : o + (n if st[s] == 0 or kind == "j" else cap[s])] = True
        assert out[o : o + n].tobytes() == xout[o : o + n].tobytes(), s
        if err == 2:  # the oracle's output exceeded the slot
            assert st[s] == ez.ENOSPC, (s, st[s])
            bad.add(s)
            continue
        assert st[s] == err, (s, st[s], err)
        assert n == len(want), (s, n, len(want))
        assert out[o : o + n].tobytes() == want, s
        if err != 0:
            bad.add(s)
    for name, a in (("K2" + kind, out), ("exact", xout)):
        stray = np.flatnonzero(~inside & (a != 0xA5))
        assert stray.size == 0, (name, stray[:8], ooff[:4])
    if handed is not None:
        got = set(int(x) for x in w[1 : 1 + int(w[0])])
        assert int(w[0]) == len(got)
        expect = bad if handed == "auto" else (set(range(count)) if handed == "all" else set(handed))
        assert got == expect, (sorted(got), sorted(expect))
    assert np.array_equal(whole.cpu().numpy()[GUARD + pad : GUARD + pad + total_in], np.frombuffer(b"".join(ins), np.uint8)), "the input was written"
    nh, _, nd, _ = k2_lists(left, count)
    return left, nh, (nd if fast in ("t", "w") else 0)  # (K2r and K2j defer nothing: the word is not theirs)
