"""K2t's steps (eazy_amd/csrc/ez_k2_tok.h: the advances, the segment exits and the exits two steps on,
the walk's step, the marking and the entries of stepped-over segments; the round's parse, cut, copy
plan, redirect search and batch rule; the checks that hand over), compiled for the host by
tools/k2_tok_check.hip and run step by step as tok_one runs them, over LDS arrays of the kernel's
sizes, on hand-built streams: every header form at each position before a window's end (the first
window and a drifted one) and at each residue of a lane segment, rare forms back to back and in a
landing's segment, token-like literal bodies, padding, the exit clamp, lengths around a window,
invalid forms; rounds of 63, 64 and 65 tokens, tokens around kTBig, rounds around both budgets,
resets, distances, slots, copy sources around the batch rule, 64 chained copies, the redirect search
on both sides of its threshold and one to three redirects deep; every stream cut at each of its last
27 bytes.  Per window the token starts, the next entry and the verdict equal one in-order walk; per
stream the bytes, with every batch's copies run in lane order and in reverse, equal the oracle's
Reader.  CPU only; the program exits non-zero at its first mismatch and prints the stream."""

import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON + k2_check_build.csrc("ez_k2_tok.h", "ez_k2_ring.h", "ez_wave.h", "ez_internal.h")

# the classes the program counts: each must have been visited
CLASSES = ("runs", "windows", "taken", "handed_error", "handed_design", "seams", "residues", "rare_pairs", "rare_steps", "exit2_stops",
           "stepped_over", "empty_segments", "pad_windows", "clamped", "bodies", "lengths", "cuts", "cuts_taken", "cuts_handed_ok", "invalid",
           "walk_handed", "rounds", "nr63", "nr64", "alone", "cut_big", "cut_budget", "budget_edges", "reset_off_lane0", "code4", "code5",
           "code6", "code7", "code8", "room_alone", "slots", "batches", "chain64", "searches", "below_threshold", "in_literal", "redirect1",
           "redirect2", "unresolved", "straddle", "zero_len", "source_edges", "short_period", "deferred")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return k2_check_build.build_check("k2_tok_check", tmp_path_factory.mktemp("k2_tok"), HEADERS)


def test_tok_steps_match_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    assert counts["seams"] == 2 * sum(min(n, 16) + 1 for n in FORM_BYTES)  # both windows, every form, every position
    assert counts["residues"] == 16 * len(FORM_BYTES)
    assert counts["chain64"] >= 2 * 4  # 64 batches in a round: four streams, both budgets
    assert counts["code7"] + counts["room_alone"] == 2 * counts["slots"]  # every short slot, both budgets
    assert p.stdout.rstrip().endswith("ok")


# the byte lengths of tools/k2_check_common.h forms(), in its order
FORM_BYTES = (51, 202, 1003, 70005, 2, 3, 4, 4, 5, 6, 7, 3, 2, 2, 3, 6, 1, 15, 16, 17, 40)
