"""The end-to-end cases of the paired-end tests (tests/test_pairs_model.py shows on the CPU that each reaches every fate; tests/test_gpu_pairs.py
runs them on the GPU): 2 000 pairs, fragments of 100-400 bases, mates of 75, 1 % substitutions, some junk mates and chimeric pairs."""
import helpers
import pairs_model as pm

pa = helpers.pa
N_PAIRS = 2000
# name -> (index, orientation, seed)
CASES = {"gencode_k20_fr": ("small20", "fr", 11), "gencode_k31_rf": ("small31", "rf", 12), "synth400_k24_ff": ("synth24", "ff", 13),
         "gencode_k20_ff": ("small20", "ff", 14), "synth400_k24_fr": ("synth24", "fr", 15), "gencode_k31_fr": ("small31", "fr", 16)}
_hosts = {}


def host_of(key, small_index=None):
    if key not in _hosts:
        if key.startswith("small"):
            k = int(key[5:])
            _hosts[key] = small_index(k) if small_index else pa.build_index(str(helpers.FASTA), k, 8)
        else:
            _hosts[key] = pa.HostIndex.from_txome(pa.Txome.synthesize(120, 400, 5), 24, 8)
    return _hosts[key]


_cases = {}


def case(name, small_index=None):
    """-> (host index, mates 1, mates 2, orientation)"""
    if name not in _cases:
        key, orient, seed = CASES[name]
        host = host_of(key, small_index)
        r1, r2, _ = pm.simulate_pairs(pm.transcripts_text(host), N_PAIRS, seed, sub_rate=0.01, orient=orient, junk_every=50, chimera_every=10)
        _cases[name] = (host, r1, r2, orient)
    return _cases[name]
