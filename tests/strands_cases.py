"""The end-to-end cases of the unstranded tests: pairs simulated as "fr" (fragments of 100-400 bases, mates of 75, 1 % substitutions, some junk
mates and chimeric pairs) with the mates of every odd pair swapped. tests/test_strands_model.py shows on the CPU that the antisense case reaches
every fate of the rule; tests/test_gpu_strands.py runs the cases on the GPU."""
import helpers
import pairs_cases
import pairs_model as pm
import strands_model as sm

pa = helpers.pa
# name -> (index, pairs, seed)
CASES = {"anti_gencode_k20": ("anti20", 2000, 21), "gencode_k31": ("small31", 2000, 22), "synth400_k24": ("synth24", 2000, 23)}
_hosts, _cases = {}, {}


def host_of(key, small_index=None):
    if key not in _hosts:
        _hosts[key] = sm.antisense_index(pairs_cases.host_of("small20", small_index), 20) if key == "anti20" else pairs_cases.host_of(key, small_index)
    return _hosts[key]


def pairs_of(host, n, seed):
    r1, r2, _ = pm.simulate_pairs(pm.transcripts_text(host), n, seed, sub_rate=0.01, junk_every=50, chimera_every=10)
    return sm.unstranded(r1, r2)


def case(name, small_index=None):
    """-> (host index, mates 1, mates 2)"""
    if name not in _cases:
        key, n, seed = CASES[name]
        host = host_of(key, small_index)
        _cases[name] = (host,) + pairs_of(host, n, seed)
    return _cases[name]
