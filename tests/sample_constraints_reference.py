"""Plain reference of constrained sampling (include/sat_hip.h, `sat_sample_filtered_ex`): numpy on the CPU, one obvious line per
rule, nothing shared with the code under test.  The row x becomes x' -- the repetition penalty on every prefix token, -inf on every
banned token (`beam_constraints_reference.banned_tokens`: the four rules of the constrained beam) -- and the draw and its
log-probability are `sample_reference`'s on x'."""
import numpy as np

import beam_constraints_reference as BC
import sample_reference as R


class Rules:
    def __init__(self, suppress_ids=(), min_length=0, no_repeat_ngram=0, block_repeat=False, repetition_penalty=1.0, end_id=None):
        self.suppress_ids, self.min_length, self.no_repeat_ngram = tuple(suppress_ids), min_length, no_repeat_ngram
        self.block_repeat, self.repetition_penalty, self.end_id = block_repeat, repetition_penalty, end_id

    def kw(self):
        return dict(suppress_ids=self.suppress_ids, min_length=self.min_length, no_repeat_ngram=self.no_repeat_ngram,
                    block_repeat=self.block_repeat, repetition_penalty=self.repetition_penalty, end_id=self.end_id)


def banned(prefix, V, end_id=None, suppress_ids=(), min_length=0, no_repeat_ngram=0, block_repeat=False):
    """the banned columns of a row with this prefix at step len(prefix); a prefix token outside [0, V) is "no token" (-1)"""
    prefix = [int(y) if 0 <= int(y) < V else -1 for y in prefix]
    return set(v for v in BC.banned_tokens(prefix, end_id, suppress_ids, min_length, no_repeat_ngram, block_repeat) if 0 <= v < V)


def transform(x, prefix, end_id=None, suppress_ids=(), min_length=0, no_repeat_ngram=0, block_repeat=False, repetition_penalty=1.0):
    """x f32 [V], prefix y_0..y_{t-1} -> x' f32 [V]"""
    x = np.array(x, dtype=np.float32)
    theta = np.float32(repetition_penalty)
    with np.errstate(invalid="ignore"):
        for v in set(int(y) for y in prefix if 0 <= int(y) < len(x)):                 # each seen token once
            x[v] = x[v] / theta if x[v] > 0 else x[v] * theta                         # one f32 operation, correctly rounded
    for v in banned(prefix, len(x), end_id, suppress_ids, min_length, no_repeat_ngram, block_repeat):
        x[v] = -np.inf                                                                # a ban wins over the penalty
    return x


def transform_rows(x, prefixes, rules):
    """x [R, V], prefixes [R, >= t] (the first t columns count) or None at t = 0"""
    return np.stack([transform(x[r], [] if prefixes is None else prefixes[r], **rules.kw()) for r in range(len(x))])


def reference(xp, tau, k, p, seed, t, rank, r):
    """(n, clearance, token, margin, logp, order) of one TRANSFORMED row, as tests/test_gpu_sample.py's `reference`; a row without a
    candidate: (0, inf, 0, inf, -inf, [])"""
    order, n, clr = R.kept_prefix(xp, tau, k, p)
    if len(order) == 0:
        return 0, np.inf, 0, np.inf, -np.inf, order
    tok, margin = R.draw(xp, tau, order[:n], seed, rank, r, t)
    return n, clr, tok, margin, R.logp(xp, tau, order[:n], tok), order


# ---- the single-step sweep both test files enumerate (the host file checks its excuse caps, the GPU file runs it) --------------------
VS = [5, 63, 64, 65, 257, 1025, 4099, 12289]
RS = [1, 3, 65]
TS = [0, 1, 2, 3, 7, 19, 63]
SETTINGS = [(1.0, 0, 1.0), (0.7, 5, 1.0), (1.0, 0, 0.9), (1.7, 64, 0.35)]           # (tau, top_k, top_p)
CHECKED = {1: [0], 3: [0, 2], 65: [0, 2, 64]}                                      # the rows compared with the numpy reference, by R
GEN_SEED, SEED, RANK, END_ID, PREFIX_STRIDE = 2025, 0x0FEDCBA987654321, 1, 2, 64
BAND, CLOSE = 1e-6, 1e-4                                                            # the two excuses of tests/test_gpu_sample.py
RULE_SETS = [
    ("suppress", Rules(suppress_ids=(0, 1, 3))),
    ("min_length", Rules(min_length=5, end_id=END_ID)),
    ("block_repeat", Rules(block_repeat=True)),
    ("ngram1", Rules(no_repeat_ngram=1)),
    ("ngram2", Rules(no_repeat_ngram=2)),
    ("ngram3", Rules(no_repeat_ngram=3)),
    ("all", Rules(suppress_ids=(0, 1, 3), min_length=5, end_id=END_ID, no_repeat_ngram=3, block_repeat=True, repetition_penalty=1.3)),
    ("theta1.3", Rules(repetition_penalty=1.3)),
    ("theta0.8", Rules(repetition_penalty=0.8)),
]
_CACHE = {}


def pad4(v):
    return (v + 3) // 4 * 4


def ldls_of(V):
    return [V, pad4(V), pad4(V) + 4]


def sweep_rows(V):
    """f32 [65, V], normal(0, 2.5)"""
    if ("rows", V) not in _CACHE:
        _CACHE[("rows", V)] = np.random.default_rng(GEN_SEED + V).normal(0.0, 2.5, (65, V)).astype(np.float32)
    return _CACHE[("rows", V)]


def alphabet(V):
    """at most 6 columns the prefixes are drawn from, so that n-grams repeat: the first columns, the middle, the last whole
    16-byte chunk's end and the V % 4 tail's"""
    return sorted(set(c for c in (0, 2, 3, V // 2, pad4(V) - 5, V - 1) if 0 <= c < V))


def sweep_prefixes(V):
    """i64 [65, PREFIX_STRIDE] over alphabet(V); the first t columns are the prefix at step t"""
    if ("prefix", V) not in _CACHE:
        rng = np.random.default_rng(GEN_SEED + 7 * V)
        _CACHE[("prefix", V)] = np.asarray(alphabet(V), dtype=np.int64)[rng.integers(0, len(alphabet(V)), (65, PREFIX_STRIDE))]
    return _CACHE[("prefix", V)]


def sweep_cases():
    """(V, ldl, R, t, rule name, Rules, (tau, k, p)): every (V, t, rule set, setting); the nine (ldl, R) pairs of a V rotate so
    that each pair meets 28 of a V's 252 cases, among them every t, every rule set and every setting"""
    out = []
    for V in VS:
        pairs = [(ldl, R_) for ldl in ldls_of(V) for R_ in RS]
        for ti, t in enumerate(TS):
            for ri, (name, rules) in enumerate(RULE_SETS):
                for si, setting in enumerate(SETTINGS):
                    ldl, R_ = pairs[(ri + ti + 7 * si) % 9]
                    out.append((V, ldl, R_, t, name, rules, setting))
    return out


def sweep_transformed(V, t, name, rules):
    """x' f32 [65, V] of the sweep's rows under the rule set at step t"""
    if ("xp", V, t, name) not in _CACHE:
        _CACHE[("xp", V, t, name)] = transform_rows(sweep_rows(V), sweep_prefixes(V)[:, :t], rules)
    return _CACHE[("xp", V, t, name)]


def sweep_references():
    """{(V, t, rule name, setting, r): reference(...)} for the checked rows of every case, computed once per process"""
    if "refs" not in _CACHE:
        refs = {}
        for (V, ldl, R_, t, name, rules, (tau, k, p)) in sweep_cases():
            xp = sweep_transformed(V, t, name, rules)
            for r in CHECKED[R_]:
                refs[(V, t, name, (tau, k, p), r)] = reference(xp[r], tau, k, p, SEED, t, RANK, r)
        _CACHE["refs"] = refs
    return _CACHE["refs"]


def sweep_excuses():
    """(rows checked, rows in the nucleus rounding band, rows with a close draw, rows without a candidate) -- on the reference alone"""
    refs = sweep_references()
    return (len(refs), sum(ref[1] < BAND for ref in refs.values()), sum(ref[3] < CLOSE for ref in refs.values()),
            sum(len(ref[5]) == 0 for ref in refs.values()))


def check_properties(ids, rules, V):
    """every step of every row -- also behind an end_id -- drew a token outside its banned set; returns the number of draws"""
    ids = np.asarray(ids)
    rows = ids.reshape(-1, ids.shape[-1])
    kw = rules.kw()
    kw.pop("repetition_penalty")
    for row in rows:
        row = row.tolist()
        for i in range(len(row)):
            assert row[i] not in banned(row[:i], V, **kw), (row, i)
    return rows.size
