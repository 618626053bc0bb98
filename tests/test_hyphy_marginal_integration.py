"""ReconstructAncestors (lf, MARGINAL [, DOLEAVES]) through the real HyPhy host with HYPHY_HIP_MARGINAL=1: the adapter answers
RecoverAncestralSequencesMarginal with ONE hyphy_hip_marginal_ancestral call instead of I*(D-1) (L*D) pinned evaluations.  The
support matrix the host leaves behind and the reconstructed alignment are compared with the unmodified reference binary's."""
import os
import re
import tempfile

import numpy as np
import pytest

from tests.test_hyphy_integration import ENV, HIP_BIN, _case, _device_calls, _need_binaries

pytestmark = pytest.mark.gpu

MENV = dict(ENV, HYPHY_HIP_MARGINAL="1")
NUM = re.compile(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?")


def _marginal_calls(stdout):
    m = re.findall(r"\[hyphy_hip\] (\d+) marginal reconstructions ran on the device", stdout)
    return max(int(x) for x in m) if m else 0


def _run(case, binary, env, leaves=False, optimize=False):
    from oracle import hbl
    tmp = tempfile.mkdtemp(prefix="marg_")
    fasta, outp, ancp, supp = (os.path.join(tmp, n) for n in ("aln.fasta", "out.txt", "anc.txt", "support.txt"))
    hbl.write_fasta(fasta, case["names"], case["seqs"])
    txt = hbl.build_script(fasta=fasta, newick=case["newick"], unit=case["unit"], model_block=case["model_block"],
                           model_name=case["model_name"], globals_=case["globals_"], branch_t=case["branch_t"],
                           out_path=outp, per_site=False, category=case.get("category"))
    tail = ""
    if optimize:
        tail += "OPTIMIZATION_PRECISION = 0.001; VERBOSITY_LEVEL = -1;\nOptimize (m2_, lf);\n"
    tail += ("DataSet anc = ReconstructAncestors (lf, MARGINAL" + (", DOLEAVES" if leaves else "") + ");\n"
             "DataSetFilter af = CreateFilter (anc, 1);\nDATA_FILE_PRINT_FORMAT = 9;\n"
             f'fprintf ("{ancp}", CLEAR_FILE, af);\n'
             f'fprintf ("{supp}", CLEAR_FILE, anc.marginal_support_matrix);\n')
    assert txt.count("LFCompute (lf, LF_DONE_COMPUTE);\n") == 1
    txt = txt.replace("LFCompute (lf, LF_DONE_COMPUTE);\n", tail + "LFCompute (lf, LF_DONE_COMPUTE);\n")
    out = hbl.run_script(txt, tmp, binary=binary, extra_env=env)
    sup = np.array([float(x) for x in NUM.findall(open(supp).read())])
    return open(ancp).read(), sup, out


CAT = dict(name="rc", weights=[0.7, 0.25, 0.05], values=[0.1, 1.0, 5.0])


@pytest.mark.parametrize("leaves", [False, True], ids=["internal", "doleaves"])
@pytest.mark.parametrize("which", ["codon", "nuc", "codon_cat3"])
def test_marginal_support_matches_reference(which, leaves):
    _need_binaries()
    case = {"codon": lambda: _case("codon", 8, 40, 11), "nuc": lambda: _case("nuc", 8, 300, 21),
            "codon_cat3": lambda: _case("codon", 8, 40, 11, category=CAT)}[which]()
    anc_cpu, sup_cpu, _ = _run(case, None, None, leaves)
    anc_gpu, sup_gpu, out = _run(case, HIP_BIN, MENV, leaves)
    assert _marginal_calls(out) == 1, out[-600:]
    assert _device_calls(out) < 10, out[-600:]
    assert len(sup_cpu) > 100 and sup_gpu.shape == sup_cpu.shape
    assert np.allclose(sup_gpu, sup_cpu, rtol=1e-9, atol=1e-14), np.max(np.abs(sup_gpu - sup_cpu))
    assert len(anc_cpu) > 100 and anc_gpu == anc_cpu


def test_marginal_after_optimize_uses_device_matrices():
    """After Optimize (adapter mode B: the exponentials were formed on the device), the one-pass answer equals the device's own
    pinned route over the same fit, and the reconstructed alignment equals the unmodified reference's."""
    _need_binaries()
    case = _case("codon", 8, 40, 11)
    anc_cpu, _, _ = _run(case, None, None, optimize=True)
    anc_pin, sup_pin, out_pin = _run(case, HIP_BIN, ENV, optimize=True)
    anc_one, sup_one, out_one = _run(case, HIP_BIN, MENV, optimize=True)
    assert _marginal_calls(out_pin) == 0 and _marginal_calls(out_one) == 1
    assert re.search(r"(\d+) matrix exponentials moved to the device", out_one)
    assert _device_calls(out_pin) - _device_calls(out_one) > 300
    assert np.allclose(sup_one, sup_pin, rtol=1e-9, atol=1e-14), np.max(np.abs(sup_one - sup_pin))
    assert len(anc_cpu) > 100 and anc_one == anc_pin == anc_cpu
