"""Dirty scratch as a test input: what a route's workspace and the library's cached scratch hold
when a call starts.

A workspace lies between two guards of GUARD bytes of SENT (guarded, guards_intact) and starts as a
fill byte or as a copy of what an earlier call left (a tensor).  The library's own scratch is set
with ez.fill_cached, or left as a decoy call of the same geometry left it.  under() runs one target
in one of the four STATES and holds the conditions that keep the test from passing vacuously: the
scratch exists before it is dirtied, the fill covers it, and the target runs in the very buffers
that were dirtied (ez.fill_cached(-1) reports the same total before and after: a cache entry that
grows is freed and allocated anew)."""

import numpy as np

GUARD = 64  # bytes of SENT on both sides of a workspace
SENT = 0x3C
STATES = ("zero", "stale", "a5", "ff")  # in the order they run
FILL = {"zero": 0x00, "a5": 0xA5, "ff": 0xFF}

COVERED = {}  # {what: bytes ez.fill_cached covered}, printed by the tests (-s shows it)


def guarded(cuda, nbytes, init=0):
    """-> (whole, view): a workspace of nbytes between two guards.  init: a fill byte, or a uint8
    tensor whose first bytes are copied in (the rest, if it is shorter, is 0)."""
    import torch

    whole = torch.full((GUARD + nbytes + GUARD,), SENT, dtype=torch.uint8, device=cuda)
    view = whole[GUARD : GUARD + nbytes]
    assert view.data_ptr() % 16 == 0
    if isinstance(init, int):
        view.fill_(init)
    else:
        view.zero_()
        n = min(nbytes, init.numel())
        view[:n].copy_(init.reshape(-1).view(torch.uint8)[:n])
    return whole, view


def guards_intact(whole, what=""):
    w = whole.cpu().numpy()
    assert (w[:GUARD] == SENT).all(), f"{what}: bytes before the workspace written"
    assert (w[-GUARD:] == SENT).all(), f"{what}: bytes after the workspace written"


def k2_lists(ws, count):
    """Of an ez_decompress_workspace(count) as a batch decode left it -> (streams handed over, their
    list's words [1 .. count], deferred literals, the deferred records' words)."""
    w = ws.cpu().numpy().view(np.uint32)
    d = 2 * count + 32
    return int(w[0]), w[1 : 1 + count], int(w[d]), w[d + 4 :]


def assert_decoy_left_more(decoy_ws, count, handed, deferred, defers):
    """The decoy's workspace holds longer lists than the target will write (handed, deferred: the
    target's counts), and non-zero words past the target's list ends."""
    h, hl, d, dl = k2_lists(decoy_ws, count)
    assert h > handed, f"the decoy handed over {h} streams, the target {handed}"
    assert hl[handed:h].any(), "no stale hand-over entry past the target's list"
    if defers:
        assert d > deferred, f"the decoy deferred {d} literals, the target {deferred}"
        assert dl[6 * deferred : 6 * d].any(), "no stale deferred-literal record past the target's list"


def under(state, target, decoy=None, scratch=True, what=None):
    """Run target(ws_init) with the library's scratch and the workspace in `state`.

    target(ws_init) runs the route once, checks it against the oracle and returns what the stale
    state needs of it (see decoy); ws_init is the workspace's initial contents (guarded's init).
    decoy(first) (the stale state) runs the decoy call(s) of the target's geometry, asserts that
    they took the target's route and left more behind than the target writes (first: what the warm
    target call returned), and returns the workspace they left (None where the route has none).
    scratch: the route's launcher keeps scratch in the library's caches."""
    import eazy_amd as ez

    ez.release_cached()
    first = target(0)  # warm: the cache entries of this geometry exist (and the control's control)
    if state == "stale":
        ws_init = decoy(first)
        if ws_init is None:
            ws_init = 0
    else:
        covered = ez.fill_cached(FILL[state])
        assert covered > 0 or not scratch, "fill_cached covered nothing: the route's scratch is not in a cache"
        ws_init = FILL[state]
    before = ez.fill_cached(-1)
    assert before > 0 or not scratch, "the route keeps no scratch in a cache"
    target(ws_init)
    after = ez.fill_cached(-1)
    assert after == before, f"the target did not run in the dirtied scratch: {before} bytes cached before it, {after} after"
    if what is not None:
        COVERED[what] = before
        print(f"fill_cached covers {before} bytes: {what}")
    return before
