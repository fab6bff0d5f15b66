"""The model of the unstranded stage, written from the rule in include/pseudoaligner_amd.h ("unstranded libraries"), not from the stage (the rule of csrc/strands.hip over the skeleton of csrc/pair_stage.hpp):

  * the merge rule over two candidates of an item (pairs_model mates: None | (sorted id list, coverage, mismatches));
  * its stats vector and the two identities;
  * unstranded(r1, r2): the mates of every odd pair swapped — what an unstranded protocol does to an "fr" library;
  * antisense_index(host, k): the transcripts of `host` plus the reverse complement of every 7th one as extra transcripts, so that both
    candidates of many items map and the rule's both-mapped rows are reached;
  * the whole model on text: pairs (four oracle mappings, the pair rule twice, the merge) and single reads.
All integers: the tests compare with equality."""
import numpy as np

import helpers
import pairs_model as pm

pa = helpers.pa
STAT_NAMES = ("items", "both_mapped", "sense_only", "antisense_only", "neither", "ties", "by_reference", "in_arena")


def key_of(c):
    """(class non-empty, coverage, -mismatches) of a mapped candidate"""
    return (1 if c[0] else 0, c[1], -c[2])


def merge_rule(s, r):
    """two candidates -> (result, fate); result None | (ids, coverage, mismatches); fate one of "neither", "sense_only",
    "antisense_only", "sense_wins", "antisense_wins", "tie" """
    if s is None and r is None:
        return None, "neither"
    if r is None:
        return (list(s[0]), s[1], s[2]), "sense_only"
    if s is None:
        return (list(r[0]), r[1], r[2]), "antisense_only"
    ks, kr = key_of(s), key_of(r)
    if ks > kr:
        return (list(s[0]), s[1], s[2]), "sense_wins"
    if kr > ks:
        return (list(r[0]), r[1], r[2]), "antisense_wins"
    return (sorted(set(s[0]) | set(r[0])), s[1], s[2]), "tie"


def merge(cand_s, cand_r):
    """-> (results RESULT_DTYPE with class_off = the CSR offset, class_offsets[n + 1], class_ids, stats dict, fate of every item)"""
    n = len(cand_s)
    assert len(cand_r) == n
    res = np.zeros(n, pm.RESULT_DTYPE)
    coff = np.zeros(n + 1, np.uint64)
    ids_all, fates = [], []
    st = dict.fromkeys(STAT_NAMES, 0)
    st["items"] = n
    for i, (s, r) in enumerate(zip(cand_s, cand_r)):
        out, fate = merge_rule(s, r)
        fates.append(fate)
        st[{"sense_wins": "both_mapped", "antisense_wins": "both_mapped", "tie": "both_mapped"}.get(fate, fate)] += 1
        st["ties"] += fate == "tie"
        if out is not None:
            ids, cov, mm = out
            assert ids == sorted(set(ids))
            res[i] = (cov, mm | pm.MAPPED_BIT, len(ids_all), len(ids))
            ids_all.extend(ids)
        coff[i + 1] = len(ids_all)
    return res, coff, np.array(ids_all, np.uint32), st, fates


def check_stats(stats, results):
    """the two identities of the header"""
    assert stats["items"] == stats["both_mapped"] + stats["sense_only"] + stats["antisense_only"] + stats["neither"]
    mapped = (results["mismatches"] >> 31).astype(bool)
    empty = int((mapped & (results["class_len"] == 0)).sum())
    assert stats["by_reference"] + stats["in_arena"] == stats["items"] - stats["neither"] - empty


def candidates_from_results(res, coff, ids):
    """the model's (or map_pairs') CSR results -> candidates"""
    coff = np.asarray(coff, np.int64)
    return [None if not (int(res["mismatches"][i]) >> 31) else (np.asarray(ids)[coff[i]:coff[i + 1]].tolist(), int(res["coverage"][i]), int(res["mismatches"][i]) & 0x7FFFFFFF)
            for i in range(len(res))]


# ---- reads and indexes ----
def unstranded(r1, r2):
    """the mates of every odd pair swapped: pair i is read from the other strand"""
    a, b = list(r1), list(r2)
    for i in range(1, len(a), 2):
        a[i], b[i] = b[i], a[i]
    return a, b


def antisense_index(host, k):
    """the transcripts of `host` and, behind them, the reverse complement of transcripts 0, 7, 14, ... as transcripts of their own"""
    packed, tx_start = host.transcripts()
    tx_start = tx_start.astype(np.int64)
    codes = helpers.unpack_bases(packed, int(tx_start[-1]))
    parts, starts = [codes], tx_start.tolist()
    for t in range(0, len(tx_start) - 1, 7):
        rc = pm.revcomp_codes(codes[tx_start[t]:tx_start[t + 1]])
        parts.append(rc)
        starts.append(starts[-1] + len(rc))
    return pa.HostIndex.build_packed(helpers.pack_bases(np.concatenate(parts)), np.array(starts, np.uint64), k, 8)


def _oracle_mates(oracle, reads, rc, allowed):
    tiles, lens, wpr = helpers.pack_reads_tiles(reads)
    if rc:
        tiles = pm.revcomp_tiles(tiles, lens, wpr)
    o_res, coff, ids, _ = oracle.map_tiles(tiles, lens, wpr, allowed, 4)
    return pm.mates_from_oracle(o_res, coff, ids)


def model_pairs_unstranded(host, reads1, reads2, allowed=2):
    """pairs of an unstranded library: S = the pair rule on (mate 1, revcomp mate 2), R = on (revcomp mate 1, mate 2), merged.
    -> (results, class_offsets, class_ids, stats, fates, candidates S, candidates R)"""
    oracle = helpers.Oracle(host)
    f1, r1 = _oracle_mates(oracle, reads1, False, allowed), _oracle_mates(oracle, reads1, True, allowed)
    f2, r2 = _oracle_mates(oracle, reads2, False, allowed), _oracle_mates(oracle, reads2, True, allowed)
    cs = [pm.pair_rule(a, b) for a, b in zip(f1, r2)]
    cr = [pm.pair_rule(a, b) for a, b in zip(r1, f2)]
    return merge(cs, cr) + (cs, cr)


def model_reads(host, reads, strand="both", allowed=2):
    """single reads: "fwd" as given, "rev" reverse-complemented, "both" the two merged -> (results, class_offsets, class_ids, stats, fates)"""
    oracle = helpers.Oracle(host)
    none = [None] * len(reads)
    cs = _oracle_mates(oracle, reads, False, allowed) if strand != "rev" else none
    cr = _oracle_mates(oracle, reads, True, allowed) if strand != "fwd" else none
    return merge(cs, cr)


def table_and_novel(res, coff, ids, host):
    return helpers.counts_reference(res, coff, ids, host), helpers.novel_reference(res, coff, ids, host)


def fate_counts(fates, cs, cr, res, coff):
    """the fates of the issue's table: the six of merge_rule with "tie" split by whether the union is larger than either list"""
    out = {}
    coff = np.asarray(coff, np.int64)
    for i, f in enumerate(fates):
        if f == "tie":
            n = int(coff[i + 1] - coff[i])
            f = "tie_union_larger" if n > len(cs[i][0]) and n > len(cr[i][0]) else "tie_equal_lists" if cs[i][0] == cr[i][0] else "tie_nested"
        out[f] = out.get(f, 0) + 1
    return out
