"""Same decisions as before the dispatch plan: the grid of scripts/record_dispatch_table.py runs through the public API and every name it
reports — the factorization kernel, the consumer kernel before and after a later lexls_lse_solve (which fails where no factor was kept),
lexls_lse_prefix_reuse_ready, the LexLSI batch's kernel — equals tests/dispatch_table.json, recorded once on the commit before
lexls_dispatch.h existed.  The handle state that used to be read off kernel names (resume state, factor in HBM, reciprocal solve) shows in
those observations."""
import json

import pytest

from scripts import record_dispatch_table as R

pytestmark = pytest.mark.gpu


def test_every_grid_entry_dispatches_as_recorded(hip):
    with open(R.TABLE) as f:
        t = json.load(f)
    cus = R.cu_count()
    if cus != t["cu_count"]:
        pytest.skip(f"the table was recorded on a device with {t['cu_count']} CUs, this one has {cus}")
    assert [x["entry"] for x in t["entries"]] == R.grid()
    got = R.run_entries([R.resolve(e, cus) for e in R.grid()])
    wrong = [(x["entry"], x["expect"], g) for x, g in zip(t["entries"], got) if g != x["expect"]]
    assert not wrong, f"{len(wrong)} of {len(got)} entries differ, first: {wrong[0]}"
