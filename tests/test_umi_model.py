"""CPU tier: the model of the UMI correction (tests/umi_model.py) pinned on the hand cases of tests/umi_cases.py with their expected records written
out, against a base-by-base brute force, and tied to the cell counter's rule: where every ec and every (barcode, UMI) run has one gene, the new step
followed by the gene counter in PA_GENES_UNIQUE gives the cell counter's (cell, gene, count) entries."""
from collections import Counter

import numpy as np
import pytest

import cells_model
import genes_model as gm
import umi_cases as uc
import umi_model as um


def test_thresholds_are_the_sources():
    assert uc.thresholds_in_source() == dict(UM_BLOCK=256, UM_LANE_MAX=uc.UM_LANE_MAX, UM_LDS_CAP=uc.UM_LDS_CAP)
    assert uc.UM_LANE_MAX < uc.UM_LDS_CAP and uc.UM_LDS_CAP * 8 == 64 * 1024                # two blocks of u64 words share a CU's 160 KiB


@pytest.mark.parametrize("name", sorted(uc.HAND))
def test_hand_cases_give_the_records_written_out(name):
    case, want, want_st = uc.hand(name)
    out, st = um.correct(*case[:4], case[6], "greatest")
    assert out.tobytes() == want.tobytes()
    assert all(st[k] == v for k, v in want_st.items()), (st, want_st)
    assert st["molecules_moved"] <= st["molecules_with_neighbour"] <= st["molecules_with_hamming1"] <= st["molecules_in"] - st["molecules_inert"]
    assert st["records_out"] <= st["records_in"] and st["molecules_out"] <= st["molecules_in"]
    assert np.all(out["flags"] == 0) and np.all(out["pad"] == 0)
    keys = list(zip(out["barcode"].tolist(), out["umi"].tolist(), out["ec"].tolist()))
    assert keys == sorted(set(keys))                                                         # strictly ascending


def test_the_hand_cases_say_what_they_are_for():
    chain = um.correct(*uc.hand("chain_not_transitive")[0][:4], 4)[0]
    assert [um.unpack(u, 4) for u in chain["umi"]] == ["AAAC", "AACC"] and chain["count"].tolist() == [1, 7]      # u under v, v under w: not followed
    tie = um.correct(*uc.hand("tie_broken_by_umi")[0][:4], 4, "directional")
    assert tie[1]["molecules_moved"] == 0 and tie[1]["molecules_with_neighbour"] == 2       # 3 < 2 * 3 - 1
    big = uc.hand("n_beyond_32_bits")[0]
    clamped = big[0].copy()
    assert int(clamped["count"].astype(np.uint64)[:2].sum()) > um.CLAMP                      # the target's n needs more than 32 bits
    case, left = uc.directional_case()
    for mode in ("greatest", "directional"):
        out = um.correct(*case[:4], 4, mode)[0]
        assert [set(out["umi"][out["barcode"] == b].tolist()) for b in range(6)] == left[mode]


@pytest.mark.parametrize("mode", ["greatest", "directional"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_decisions_equal_the_brute_force_and_barcodes_are_independent(seed, mode):
    case = uc.random_case(seed)
    rec, off, ids, tx_gene, _, _, umi_len = case
    out, st = um.correct(rec, off, ids, tx_gene, umi_len, mode)
    mols = um.molecules(rec, um.gene_sets(off, ids, tx_gene))
    cells = {}
    for m in mols:
        cells.setdefault(m.barcode, {})[m.umi] = m
    for m in mols:
        assert um.decide(m, cells[m.barcode], umi_len, um.MODES[mode])[0] is um.decide_brute(m, cells[m.barcode], umi_len, um.MODES[mode])
    for b in sorted(cells)[:5]:
        alone, _ = um.correct(rec[rec["barcode"] == b], off, ids, tx_gene, umi_len, mode)
        assert alone.tobytes() == out[out["barcode"] == b].tobytes()
    assert int(out["count"].astype(np.uint64).sum()) == st["reads_in"]                       # (no count is near the clamp here)


def test_greatest_then_unique_counting_is_the_cell_counters_rule():
    """reads whose ecs have one gene each and whose (barcode, UMI) runs have one gene: umi_model (GREATEST) then genes_model (PA_GENES_UNIQUE) gives
    the (cell, gene, count) entries of cells_model's UMI step on the same reads"""
    rng = np.random.default_rng(11)
    bc_len, umi_len, num_genes = 6, 5, 5
    tx_gene = np.repeat(np.arange(num_genes, dtype=np.uint32), 2)                            # gene g = transcripts 2g, 2g + 1
    barcodes = sorted({"".join(um.BASES[x] for x in rng.integers(0, 4, bc_len)) for _ in range(12)})
    gene_of_run, r1s, mapping = {}, [], []
    for _ in range(6000):
        bc, umi = barcodes[int(rng.integers(len(barcodes)))], "".join(um.BASES[x] for x in rng.integers(0, 4, umi_len))
        g = gene_of_run.setdefault((bc, umi), int(rng.integers(num_genes)))
        ids = [[2 * g], [2 * g + 1], [2 * g, 2 * g + 1]][int(rng.integers(3))]              # three ecs per gene, one gene per ec
        r1s.append(bc + umi)
        mapping.append((True, ids))
    ecs = sorted({tuple(ids) for _, ids in mapping})
    reads = Counter((um.pack(r1[:bc_len]), um.pack(r1[bc_len:]), ecs.index(tuple(ids))) for r1, (_, ids) in zip(r1s, mapping))
    rec = np.array([(b, u, e, n, 0, 0) for (b, u, e), n in sorted(reads.items())], um.BUS_RECORD_DTYPE)
    off = np.cumsum([0] + [len(e) for e in ecs]).astype(np.uint64)
    ids = np.array([t for e in ecs for t in e], np.uint32)
    # the precondition, asserted on the inputs
    G = um.gene_sets(off, ids, tx_gene)
    assert all(len(g) == 1 for g in G)
    runs = {}
    for b, u, e in zip(rec["barcode"].tolist(), rec["umi"].tolist(), rec["ec"].tolist()):
        runs.setdefault((b, u), set()).update(G[e])
    assert all(len(s) == 1 for s in runs.values())
    want, want_st = cells_model.count(r1s, mapping, tx_gene, barcodes, bc_len, umi_len)
    assert want_st["umis_corrected"] > 100 and want_st["molecules_lost_to_conflicts"] == 0 and want_st["reads_counted"] == len(r1s)
    out, st = um.correct(rec, off, ids, tx_gene, umi_len, "greatest")
    assert st["molecules_moved"] == want_st["umis_corrected"] and st["molecules_inert"] == 0
    model = gm.Model(out, off, ids, tx_gene, num_genes, bc_len, umi_len, mode="unique")
    cell_of = {um.pack(b): i for i, b in enumerate(barcodes)}                                # the whitelist is sorted: line i = the i-th barcode
    got = sorted((cell_of[int(model.barcodes[k])], g, n) for (k, g), n in model.unique_counter().items())
    assert got == want
    plain = gm.Model(rec, off, ids, tx_gene, num_genes, bc_len, umi_len, mode="unique")     # not vacuous: without the step the counts are larger
    assert sum(plain.unique_counter().values()) == sum(n for _, _, n in want) + st["molecules_in"] - st["molecules_out"] > sum(n for _, _, n in want)
