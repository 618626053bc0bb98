#!/usr/bin/env python3
"""Golden fixtures of the joint ancestral reconstruction: the states the UNMODIFIED reference binary (oracle/_ref/hyphy) prints for
`ReconstructAncestors (lf)` and `(lf, DOLEAVES)`, next to the inputs in the other fixtures' keys.

  joint_codon_small   the generator inputs of codon_small_marginal (8 taxa x 40 codons, seed 11)
  joint_nuc_ambig     8 x 300 nucleotides with ambiguity codes and a few all-gap columns
  joint_codon_cat3    the codon case with the three-class category variable of tests/test_hyphy_marginal_integration.py

Each tests/golden/<name>.npz holds D, L, flat_parents, leaf_codes, ambig, pattern_freq, site_to_pattern, t, rev, root_freqs (codon:
omega, pos_freqs; classes: cat_weights, cat_values), node_names (internal nodes by internal index, the root last, then the leaves),
states [I + L, S] (the reference's sequences as state arrays per node name, -1 where it prints a gap), pattern_class / site_class,
margins [S] and min_margin.  Before writing, it asserts here, on the CPU: tests/joint_ref.py on oracle.expm matrices reproduces
every state of the reference, the two runs agree on the internal nodes, and every pattern's smallest decision margin is >= 1e-6,
so a last-bit difference in a matrix cannot flip a decision.  If a seed does not give that margin, change the seed, not the bar."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyphy_amd import data, models, tree  # noqa: E402
from oracle import hbl, oracle  # noqa: E402
from oracle import make_golden as mg  # noqa: E402
from tests import joint_ref as jr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-6
CAT = dict(name="rc", weights=[0.7, 0.25, 0.05], values=[0.1, 1.0, 5.0])
REV_KEYS = ("AC", "AT", "CG", "CT", "GT")


def _reference_run(case, leaves, classes):
    tmp = tempfile.mkdtemp(prefix="jointgold_")
    fasta, outp, ancp, clsp = (os.path.join(tmp, n) for n in ("aln.fasta", "out.txt", "anc.txt", "cls.txt"))
    hbl.write_fasta(fasta, case["names"], case["seqs"])
    txt = hbl.build_script(fasta=fasta, newick=case["newick"], unit=case["unit"], model_block=case["model_block"],
                           model_name=case["model_name"], globals_=case["globals_"], branch_t=case["branch_t"],
                           out_path=outp, per_site=False, category=case.get("category"))
    tail = ("DataSet anc = ReconstructAncestors (lf" + (", DOLEAVES" if leaves else "") + ");\n"
            "DataSetFilter af = CreateFilter (anc, 1);\nDATA_FILE_PRINT_FORMAT = 9;\n"
            f'fprintf ("{ancp}", CLEAR_FILE, af);\n')
    if classes:
        tail += ("ConstructCategoryMatrix (cm_, lf, CLASSES);\n"
                 f'fprintf ("{clsp}", CLEAR_FILE, Columns (cm_), "\\n");\n'
                 f'for (k_ = 0; k_ < Columns (cm_); k_ += 1) {{ fprintf ("{clsp}", cm_[k_], "\\n"); }}\n')
    mark = "LFCompute (lf, LF_DONE_COMPUTE);\n"
    assert txt.count(mark) == 1
    hbl.run_script(txt.replace(mark, tail + mark), tmp)
    seqs, name = {}, None
    for ln in open(ancp).read().split("\n"):
        ln = ln.strip()
        if ln.startswith(">"):
            name = ln[1:]
            seqs[name] = ""
        elif ln and name is not None:
            seqs[name] += ln
    cls = None
    if classes:
        vals = open(clsp).read().split()
        cls = np.array([int(round(float(x))) for x in vals[1:1 + int(vals[0])]], dtype=np.int64)
    return seqs, cls


def _state(chars, unit):
    if all(c in "-?" for c in chars):
        return -1
    return models.NUC.index(chars) if unit == 1 else models.CODON_INDEX[chars]


def make(name, kind, n_taxa, n_sites, seed, category=None, missing=0.0, gap_columns=()):
    unit = 3 if kind == "codon" else 1
    syn = data.evolve(n_taxa, n_sites, unit, seed=seed)
    flat = syn.flat
    seqs = list(syn.seqs)
    if missing > 0:
        seqs = data.inject_missing(seqs, unit, missing, seed + 1000)
    for c in gap_columns:
        seqs = [s[:c * unit] + "-" * unit + s[(c + 1) * unit:] for s in seqs]
    if kind == "codon":
        bt = mg.branch_lengths(flat, seed + 7, 0.02, 0.12)
        pi = models.f3x4_codon_freqs(mg.POS_FREQS)
        rate = "t" if category is None else f"{category['name']}*t"
        args = dict(unit=3, model_block=hbl.codon_model_block(models.mg94rev_template(mg.POS_FREQS), pi, rate_expr=rate),
                    model_name="MGM", globals_=dict(R=0.3, **mg.REV))
        rev = mg.REV
    else:
        bt = mg.branch_lengths(flat, seed + 7, 0.02, 0.2)
        pi = mg.NUC_FREQS
        rev = models.hky85_rev(0.35)
        args = dict(unit=1, model_block=hbl.nuc_model_block(mg.NUC_FREQS), model_name="NM", globals_=dict(rev))
    case = dict(names=flat.leaf_names, seqs=seqs, newick=tree.to_newick(syn.tree), branch_t=bt, category=category, **args)
    inner, _ = _reference_run(case, False, False)
    both, site_class = _reference_run(case, True, category is not None)
    pd = data.compress(seqs, unit)
    D, L, I, S = pd.D, flat.L, flat.I, pd.S
    n_sites = len(pd.site_to_pattern)
    root = [n for n in inner if n not in flat.inode_names]
    assert len(root) == 1 and len(inner) == I, (sorted(inner), flat.inode_names)
    node_names = flat.inode_names[:-1] + root + flat.leaf_names
    assert sorted(both) == sorted(node_names)
    first = np.array([int(np.flatnonzero(pd.site_to_pattern == p)[0]) for p in range(S)])
    states = np.full((I + L, S), -2, dtype=np.int64)
    for r, nm in enumerate(node_names):
        per_site = np.array([_state(both[nm][s * unit:(s + 1) * unit], unit) for s in range(n_sites)])
        assert np.array_equal(per_site, per_site[first][pd.site_to_pattern]), (name, nm, "sites of one pattern differ")
        states[r] = per_site[first]
        if r < I:
            assert inner[nm] == both[nm], (name, nm, "the run without DOLEAVES differs")
    t = np.array([bt[n] for n in flat.branch_names()])
    if kind == "codon":
        values = category["values"] if category else [1.0]
        Q = np.stack([models.mg94rev_Q_batch(t * v, 0.3, rev, mg.POS_FREQS) for v in values])
    else:
        Q = np.stack([models.nuc_rev_Q(float(tt), rev, mg.NUC_FREQS) for tt in t])[None]
    P = np.stack([oracle.expm(q, kind == "codon") for q in Q])
    pattern_class = np.zeros(S, dtype=np.int64)
    if category is not None:
        assert len(site_class) == n_sites
        assert np.array_equal(site_class, site_class[first][pd.site_to_pattern])
        pattern_class = site_class[first]
    want, margins = jr.joint_ref(D, flat.flat_parents, L, pd.leaf_codes, pd.ambig, P, pi, class_of_pattern=pattern_class)
    bad = np.argwhere(want != states)
    assert len(bad) == 0, (name, "joint_ref differs from the reference", bad[:5].tolist())
    assert margins.min() >= MARGIN, (name, "smallest margin", margins.min(), "change the seed, not the bar")
    fx = dict(kind=kind, D=D, L=L, flat_parents=flat.flat_parents, leaf_codes=pd.leaf_codes, ambig=pd.ambig,
              pattern_freq=pd.pattern_freq, site_to_pattern=pd.site_to_pattern, t=t, rev=np.array([rev[k] for k in REV_KEYS]),
              root_freqs=pi, node_names=np.array(node_names), states=states, pattern_class=pattern_class,
              site_class=pattern_class[pd.site_to_pattern], margins=margins, min_margin=margins.min(), seed=seed)
    if kind == "codon":
        fx.update(omega=0.3, pos_freqs=mg.POS_FREQS)
    if category is not None:
        fx.update(cat_weights=np.array(category["weights"]), cat_values=np.array(category["values"]))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **fx)
    print(f"{name}: S = {S}  n_ambig = {len(pd.ambig)}  unresolved states = {int((states < 0).sum())}  classes used = "
          f"{sorted(set(pattern_class.tolist()))}  smallest margin = {margins.min():.3e}")


def main():
    if not hbl.have_reference():
        raise SystemExit("oracle/_ref/hyphy is not built")
    make("joint_codon_small", "codon", 8, 40, 11)
    make("joint_nuc_ambig", "nuc", 8, 300, 21, missing=0.04, gap_columns=(3, 117, 250))
    make("joint_codon_cat3", "codon", 8, 40, 11, category=CAT)


if __name__ == "__main__":
    main()
