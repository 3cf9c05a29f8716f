"""Every entry point that takes a scratch_dev (the rows of tests/scratch_cases.py) from dirty scratch of exactly its size, at the
least alignment the header allows.  One arena per row, guard | pad | scratch | guard: the guards are 4 096 bytes of a fixed
pattern, the pad puts the scratch on a multiple of the row's alignment that is NOT a multiple of twice it, and the scratch is
exactly what the ABI's own size function names.

(a) four fills, one answer: `large` from scratch of 0x00, of 0xFF, of seeded random words and of what a run of `small` left
    there, then `small` behind `large`'s leftovers; after every run the outputs are the CPU's answer byte for byte, canaries
    included, and both guards are whole (for `small`: so is every byte of the arena behind its own, smaller, size).
(b) back to back: large, small, large on one new stream and one scratch pointer with nothing between the calls, each into
    outputs of its own, one sync behind them.
(c) the harness has teeth: a "call" whose answer is a copy of the scratch is reported by (a), and one that sets a byte behind
    the scratch is reported by the guard check -- both through the library's own copy and set calls, inside the arena."""
import numpy as np
import pytest

import scratch_cases as sx

pytestmark = pytest.mark.gpu

GUARD_BYTES, GUARD_BYTE = 4096, 0x5C


class Arena:
    def __init__(self, gpu, tmp, nbytes, align):
        self.gpu, self.nbytes, self.head = gpu, int(nbytes), GUARD_BYTES + align
        self.buf = tmp.alloc(self.head + self.nbytes + GUARD_BYTES)
        assert self.buf.ptr % (2 * align) == 0
        self.scratch = self.buf.ptr + self.head
        assert self.scratch % align == 0 and self.scratch % (2 * align) != 0
        self.host = np.full(self.head + self.nbytes + GUARD_BYTES, GUARD_BYTE, np.uint8)

    def fill(self, what):
        """The scratch set to a byte value, or to seeded random 32-bit words (`what` a Generator); the guards set anew."""
        body = self.host[self.head: self.head + self.nbytes]
        if isinstance(what, int):
            body[:] = what
        else:
            words = what.integers(0, 2**32, size=(self.nbytes + 3) // 4, dtype=np.uint32)
            body[:] = words.view(np.uint8)[: self.nbytes]
        self.gpu._call("vkmr_hip_memcpy_h2d_async", self.buf, self.host.ctypes.data, self.host.nbytes)
        self.gpu.sync()

    def written_outside(self, used=None):
        """The offsets, from the scratch's first byte, of the first bytes that changed outside the first `used` bytes of the
        scratch (all of it when None): the guards, and for a call that was promised less than the arena holds, the rest."""
        used = self.nbytes if used is None else int(used)
        now = self.gpu.download(self.buf, self.host.nbytes, dtype=np.uint8)
        self.host[self.head: self.head + used] = now[self.head: self.head + used]           # what the call left: the next call's dirt
        return (np.flatnonzero(now != self.host)[:8] - self.head).tolist()


def run(gpu, arena, enqueue, read, case, used=None, stream=None):
    """One run at the arena's scratch; what is wrong with it, as a list."""
    enqueue(arena.scratch, stream)
    gpu.sync(stream)
    problems = [("output", name, where) for name, where in sx.differences(case, read())]
    outside = arena.written_outside(used)
    return problems + ([("written outside the scratch at", outside)] if outside else [])


def four_fills(gpu, row, nbytes=sx.scratch_bytes):
    """Check (a) of one row: [(which run, what was wrong)]."""
    found = []
    with gpu.scope() as tmp:
        size = {v: nbytes(row, v) for v in sx.VARIANTS}
        arena = Arena(gpu, tmp, size["large"], row.align)
        large, small = row.prepare(gpu, tmp, "large"), row.prepare(gpu, tmp, "small")
        rng = np.random.default_rng(20240)
        for name, what in (("0x00", 0x00), ("0xFF", 0xFF), ("random words", rng)):
            arena.fill(what)
            found += [(f"large from {name}", p) for p in run(gpu, arena, *large, row.case("large"))]
        arena.fill(rng)
        found += [("small from random words", p) for p in run(gpu, arena, *small, row.case("small"), used=size["small"])]
        found += [("large from what small left", p) for p in run(gpu, arena, *large, row.case("large"))]
        found += [("small from what large left", p) for p in run(gpu, arena, *small, row.case("small"), used=size["small"])]
    return found


@pytest.mark.parametrize("row", sx.ROWS, ids=lambda r: r.name)
def test_four_fills_one_answer(gpu, row):
    found = four_fills(gpu, row)
    assert not found, found[:6]


@pytest.mark.parametrize("row", sx.ROWS, ids=lambda r: r.name)
def test_back_to_back_on_one_stream(gpu, row):
    stream = gpu.new_stream()
    with gpu.scope() as tmp:
        arena = Arena(gpu, tmp, sx.scratch_bytes(row, "large"), row.align)
        runs = [(v, row.prepare(gpu, tmp, v)) for v in ("large", "small", "large")]
        arena.fill(np.random.default_rng(20241))
        for _, (enqueue, _) in runs:
            enqueue(arena.scratch, stream)                         # nothing between them but the calls
        gpu.sync(stream)
        found = [(i, v, sx.differences(row.case(v), read())) for i, (v, (_, read)) in enumerate(runs)]
        assert not any(d for _, _, d in found), [f for f in found if f[2]][:3]
        assert not arena.written_outside()
    gpu._call("vkmr_hip_stream_destroy", stream=stream)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
PSEUDO_BYTES = {"large": 4096, "small": 1024}


def pseudo_bytes(row, variant):
    return PSEUDO_BYTES[variant]


def copies_the_scratch(variant):
    """vkmr_hip_gather_digests_async with the scratch as its source: dst[0] = the first 32 bytes of the scratch, the library's
    device-to-device copy of one cell.  "Expected": the zeros a fresh allocation tends to hold."""
    return sx.Case((PSEUDO_BYTES[variant],), {"src_dev": sx.SCRATCH, "order_dev": sx.In(np.zeros(1, np.uint32)), "n": 1, "dst_dev": sx.Out("dst", 1, np.uint32, 8)},
                   {"dst": np.zeros(8, np.uint32)})


def sets_a_byte_behind(variant):
    """vkmr_hip_memset_async of ONE byte at scratch + size: the first byte of the guard, inside the arena."""
    return sx.Case((PSEUDO_BYTES[variant],), {"dst": sx.Scratch(PSEUDO_BYTES[variant]), "value": 0x11, "bytes": 1}, {})


def test_an_answer_that_depends_on_the_scratch_is_reported(gpu):
    found = four_fills(gpu, sx.Row("vkmr_hip_gather_digests_async", "", 16, copies_the_scratch), pseudo_bytes)
    runs = {which for which, _ in found}
    assert "large from 0x00" not in runs and {"large from 0xFF", "large from random words", "small from random words"} <= runs, found
    assert all(p[0] == "output" for _, p in found), found          # and it stayed inside: the guards did not complain


def test_a_byte_behind_the_scratch_is_reported(gpu):
    found = four_fills(gpu, sx.Row("vkmr_hip_memset_async", "", 16, sets_a_byte_behind), pseudo_bytes)
    # every run, whatever the fill.  The last one names large's byte: nothing refilled the arena since, so that guard byte is still
    # damaged, while the byte behind small's own size already held the value that small sets again
    want = {"large": [PSEUDO_BYTES["large"]], "small from random words": [PSEUDO_BYTES["small"]], "small from what large left": [PSEUDO_BYTES["large"]]}
    assert len(found) == 6 and len({which for which, _ in found}) == 6, found
    assert all(p == ("written outside the scratch at", want.get(which, want["large"])) for which, p in found), found
