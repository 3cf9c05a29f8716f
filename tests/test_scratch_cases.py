"""tests/scratch_cases.py held to include/vkmr_hip.h and to the CPU, without a GPU: the table names exactly the entry points that
take a scratch_dev, every row's two variants size their scratch through the library's own size function -- small strictly below
large, both whole units of the alignment the header promises --, and every expected answer comes out of the CPU twin and is not
the canary."""
import numpy as np
import pytest

import abi_support
import scratch_cases as sx

TAKES_SCRATCH = sorted(name for name, d in abi_support.declarations().items() if any(p == "scratch_dev" for _, p in d.params))


def test_the_header_has_entry_points_with_scratch():
    assert len(TAKES_SCRATCH) >= 30 and len(sx.ROWS) == len(sx.BY_NAME)


@pytest.mark.parametrize("name", TAKES_SCRATCH)
def test_every_declaration_with_a_scratch_has_a_row(name):
    assert name in sx.BY_NAME, f"{name} takes a scratch_dev and has no row in tests/scratch_cases.py"


def test_every_row_is_a_declaration_with_a_scratch():
    assert sorted(sx.BY_NAME) == TAKES_SCRATCH


def test_at_most_two_rows_leave_cells_out_and_each_quotes_the_header():
    header = " ".join(open(abi_support.INCLUDE + "/vkmr_hip.h").read().replace(" *", " ").split())
    allowed = [row for row in sx.ROWS if row.allows]
    assert len(allowed) <= 2
    for row in sx.ROWS:
        assert all(bool(row.case(v).unspecified) == bool(row.allows) for v in sx.VARIANTS), row.name
        assert row.allows in header, row.name


@pytest.mark.parametrize("row", sx.ROWS, ids=lambda r: r.name)
def test_sizes_and_the_cpus_answer(row, native):
    small, large = sx.scratch_bytes(row, "small"), sx.scratch_bytes(row, "large")
    assert 0 < small < large, (small, large)
    assert small % row.align == 0 and large % row.align == 0, (small, large, row.align)
    assert row.align in (8, 16) and (row.align == 8) == ("_find_" in row.name)
    a, b = row.size("small"), row.size("large")
    assert len(a) == len(b) and all((x != y) != (i in row.fixed) for i, (x, y) in enumerate(zip(a, b))), (a, b)      # they differ in every argument the call leaves open
    names = [n for _, n in abi_support.declarations()[row.name].params[2:]]
    for variant in sx.VARIANTS:
        case = row.case(variant)
        assert sorted(case.args) == sorted(names), sorted(set(case.args) ^ set(names))
        outs = {v.name: v for v in case.args.values() if isinstance(v, sx.Out)}
        assert sorted(outs) == sorted(case.expected) and set(case.unspecified) <= set(outs)
        written = False
        for name, want in row.expected(variant).items():
            want, o = np.asarray(want), outs[name]
            assert want.dtype == o.dtype and want.size == o.n * o.width, (name, want.dtype, want.shape, o.n, o.width)
            written = written or (want.reshape(-1) != sx.pattern(o.dtype)).any()
        assert written, "no output differs from its canary"
