#!/usr/bin/env python3
"""Golden fixtures of the hidden-Markov rate classes: what the UNMODIFIED reference binary (oracle/_ref/hyphy) answers for a
likelihood function whose category variable carries an HMM model — `LFCompute` (SumUpHiddenMarkov) and
`ConstructCategoryMatrix (.., SHORT)` (RunViterbi) — next to the inputs in the other fixtures' keys.

  hmm_nuc_small    8 taxa x 300 nucleotides
  hmm_codon_cat3   8 taxa x 40 codons

The category line of oracle.hbl.build_script is replaced by one that carries an HMM model, in the form of
tests/hbltests/HMM/TreeHMM.bf:11-20 and libv3/models/rate_variation.bf:52-74: three classes, T[k][m] = lambda w[m] off the diagonal
(lambda = 0.15, unequal class weights), a starting vector that is not uniform.

Each tests/golden/<name>.npz holds kind, D, L, flat_parents, leaf_codes, ambig, pattern_freq, site_to_pattern, t, rev, root_freqs
(codon: omega, pos_freqs), cat_weights, cat_values, T, pi, logl, printed [n_sites], path [n_sites] and min_margin.

`printed` is the matrix the reference hands out.  It is NOT RunViterbi's path: ConstructCategoryMatrix passes that path (one entry per
site, in site order) through RemapMatrix (likefunc.cpp:1608-1649, the "just copy" branch for HMM partitions is commented out), which
reads it as if it were indexed by pattern: printed[i] = path[site_to_pattern[i]].  The library's entry point stands where RunViterbi
stands, so `path` is RunViterbi's own: hmm_ref.viterbi_mp's path, of which the reference shows the entries 0 .. S-1 (every pattern
index occurs in site_to_pattern), all of them equal.

Before writing, it asserts here, on the CPU: tests/hmm_ref.forward_mp on per-class pattern likelihoods from tests/scalefree.py
(matrices from oracle.expm) reproduces the reference's log L within 1e-9 relative; hmm_ref.viterbi_mp's path, remapped as above,
reproduces `printed` at every site, with a smallest decision margin >= 1e-6.  If a seed does not give that margin, change the seed,
not the bar."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyphy_amd import data, models, tree  # noqa: E402
from oracle import hbl, oracle  # noqa: E402
from oracle import make_golden as mg  # noqa: E402
from tests import hmm_ref  # noqa: E402
from tests import scalefree as sf  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-6
CAT = dict(name="rc", weights=[0.6, 0.3, 0.1], values=[0.2, 1.0, 4.0])
LAMBDA = 0.15
START = [0.5, 0.3, 0.2]
REV_KEYS = ("AC", "AT", "CG", "CT", "GT")


def transition_matrix(weights, lam):
    w = np.asarray(weights, dtype=np.float64)
    T = lam * np.tile(w, (len(w), 1))
    np.fill_diagonal(T, 0.0)
    np.fill_diagonal(T, 1.0 - T.sum(axis=1))
    return T


def hmm_category_lines(cat, T, start):
    C = len(cat["weights"])
    rows = "".join("{" + ",".join(repr(float(x)) for x in T[k]) + "}" for k in range(C))
    f = "".join("{" + repr(float(x)) + "}" for x in start)
    w = ",".join(repr(float(x)) for x in cat["weights"])
    v = ",".join(repr(float(x)) for x in cat["values"])
    return (f"hmm_T = {{{rows}}};\nhmm_F = {{{f}}};\nModel hmm_M = (hmm_T, hmm_F, 0);\n"
            f"category {cat['name']} = ({C}, {{{{{w}}}}}, MEAN, , {{{{{v}}}}}, 0, 1e25, , hmm_M);")


def reference_run(case, T, start):
    tmp = tempfile.mkdtemp(prefix="hmmgold_")
    fasta, outp, pathp = (os.path.join(tmp, n) for n in ("aln.fasta", "out.txt", "path.txt"))
    hbl.write_fasta(fasta, case["names"], case["seqs"])
    txt = hbl.build_script(fasta=fasta, newick=case["newick"], unit=case["unit"], model_block=case["model_block"],
                           model_name=case["model_name"], globals_=case["globals_"], branch_t=case["branch_t"],
                           out_path=outp, per_site=False, category=CAT)
    lines = txt.split("\n")
    at = [i for i, ln in enumerate(lines) if ln.startswith(f"category {CAT['name']} = ")]
    assert len(at) == 1
    lines[at[0]] = hmm_category_lines(CAT, T, start)
    txt = "\n".join(lines)
    tail = ("ConstructCategoryMatrix (cm_, lf, SHORT);\n"
            f'fprintf ("{pathp}", CLEAR_FILE, Columns (cm_), "\\n");\n'
            f'for (k_ = 0; k_ < Columns (cm_); k_ += 1) {{ fprintf ("{pathp}", cm_[k_], "\\n"); }}\n')
    mark = "LFCompute (lf, LF_DONE_COMPUTE);\n"
    assert txt.count(mark) == 1
    hbl.run_script(txt.replace(mark, tail + mark), tmp)
    logl = hbl.parse_output(outp)["logl"]
    vals = open(pathp).read().split()
    printed = np.array([int(round(float(x))) for x in vals[1:1 + int(vals[0])]], dtype=np.int8)
    return logl, printed


def make(name, kind, n_taxa, n_sites, seed):
    unit = 3 if kind == "codon" else 1
    syn = data.evolve(n_taxa, n_sites, unit, seed=seed)
    flat = syn.flat
    seqs = list(syn.seqs)
    rate = f"{CAT['name']}*t"
    if kind == "codon":
        bt = mg.branch_lengths(flat, seed + 7, 0.02, 0.12)
        pi = models.f3x4_codon_freqs(mg.POS_FREQS)
        rev = mg.REV
        args = dict(unit=3, model_block=hbl.codon_model_block(models.mg94rev_template(mg.POS_FREQS), pi, rate_expr=rate),
                    model_name="MGM", globals_=dict(R=0.3, **mg.REV))
    else:
        bt = mg.branch_lengths(flat, seed + 7, 0.02, 0.2)
        pi = mg.NUC_FREQS
        rev = models.hky85_rev(0.35)
        args = dict(unit=1, model_block=hbl.nuc_model_block(mg.NUC_FREQS, rate_expr=rate), model_name="NM", globals_=dict(rev))
    T = transition_matrix(CAT["weights"], LAMBDA)
    start = np.array(START)
    case = dict(names=flat.leaf_names, seqs=seqs, newick=tree.to_newick(syn.tree), branch_t=bt, **args)
    logl, printed = reference_run(case, T, start)
    pd = data.compress(seqs, unit)
    assert len(printed) == len(pd.site_to_pattern), (len(printed), len(pd.site_to_pattern))
    t = np.array([bt[n] for n in flat.branch_names()])
    if kind == "codon":
        Q = np.stack([models.mg94rev_Q_batch(t * v, 0.3, rev, mg.POS_FREQS) for v in CAT["values"]])
    else:
        Q = np.stack([np.stack([models.nuc_rev_Q(float(tt) * v, rev, mg.NUC_FREQS) for tt in t]) for v in CAT["values"]])
    P = np.stack([oracle.expm(q, kind == "codon") for q in Q])
    per = sf.prune(pd.D, flat.flat_parents, flat.L, pd.leaf_codes, pd.ambig, pd.pattern_freq, P, pi, weights=np.array(CAT["weights"]))
    l = np.exp(per["class_site_logl"])
    c = np.zeros(l.shape, dtype=np.int64)
    want = hmm_ref.to_float(hmm_ref.forward_mp(l, c, T, start, pd.site_to_pattern))
    assert abs(want - logl) <= 1e-9 * abs(logl), (name, "forward_mp differs from the reference", want, logl)
    margin = hmm_ref.margins(l, c, T, start, pd.site_to_pattern)
    assert margin >= MARGIN, (name, "smallest margin", margin, "change the seed, not the bar")
    path = hmm_ref.viterbi_mp(l, c, T, start, pd.site_to_pattern)
    assert sorted(set(pd.site_to_pattern.tolist())) == list(range(pd.S)) and pd.S <= len(path)
    remapped = path[pd.site_to_pattern]
    assert np.array_equal(remapped, printed), (name, "viterbi_mp differs from the reference", np.flatnonzero(remapped != printed)[:8].tolist())
    fx = dict(kind=kind, D=pd.D, L=flat.L, flat_parents=flat.flat_parents, leaf_codes=pd.leaf_codes, ambig=pd.ambig,
              pattern_freq=pd.pattern_freq, site_to_pattern=pd.site_to_pattern, t=t, rev=np.array([rev[k] for k in REV_KEYS]),
              root_freqs=pi, cat_weights=np.array(CAT["weights"]), cat_values=np.array(CAT["values"]), T=T, pi=start,
              logl=logl, printed=printed, path=path, min_margin=margin, seed=seed)
    if kind == "codon":
        fx.update(omega=0.3, pos_freqs=mg.POS_FREQS)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **fx)
    print(f"{name}: sites = {len(path)}  patterns = {pd.S}  log L = {logl!r}  |forward_mp - reference| / |log L| = "
          f"{abs(want - logl) / abs(logl):.2e}  classes on the path = {sorted(set(path.tolist()))}  switches = "
          f"{int((np.diff(path) != 0).sum())}  smallest margin = {margin:.3e}")


def main():
    if not hbl.have_reference():
        raise SystemExit("oracle/_ref/hyphy is not built")
    make("hmm_nuc_small", "nuc", 8, 300, 21)
    make("hmm_codon_cat3", "codon", 8, 40, 11)


if __name__ == "__main__":
    main()
