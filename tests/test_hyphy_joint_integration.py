"""ReconstructAncestors (lf [, DOLEAVES]) through the real HyPhy host with HYPHY_HIP_JOINT=1: the adapter answers
_TheTree::RecoverAncestralSequences with ONE hyphy_hip_joint_ancestral call per partition (the upward loop is skipped, the traceback
reads the device's state table).  The printed alignment is compared character for character with the unmodified reference binary's."""
import os
import re
import tempfile

import pytest

from tests.test_hyphy_integration import ENV, HIP_BIN, _case, _device_calls, _need_binaries

pytestmark = pytest.mark.gpu

JENV = dict(ENV, HYPHY_HIP_JOINT="1")
OFF = dict(ENV, HYPHY_HIP_JOINT="0")
CAT = dict(name="rc", weights=[0.7, 0.25, 0.05], values=[0.1, 1.0, 5.0])


def _joint_calls(stdout):
    m = re.findall(r"\[hyphy_hip\] (\d+) joint reconstructions ran on the device", stdout)
    return max(int(x) for x in m) if m else 0


def _run(case, binary, env, leaves=False, optimize=False):
    from oracle import hbl
    tmp = tempfile.mkdtemp(prefix="joint_")
    fasta, outp, ancp = (os.path.join(tmp, n) for n in ("aln.fasta", "out.txt", "anc.txt"))
    hbl.write_fasta(fasta, case["names"], case["seqs"])
    txt = hbl.build_script(fasta=fasta, newick=case["newick"], unit=case["unit"], model_block=case["model_block"],
                           model_name=case["model_name"], globals_=case["globals_"], branch_t=case["branch_t"],
                           out_path=outp, per_site=False, category=case.get("category"))
    tail = ""
    if optimize:
        tail += "OPTIMIZATION_PRECISION = 0.001; VERBOSITY_LEVEL = -1;\nOptimize (m2_, lf);\n"
    tail += ("DataSet anc = ReconstructAncestors (lf" + (", DOLEAVES" if leaves else "") + ");\n"
             "DataSetFilter af = CreateFilter (anc, 1);\nDATA_FILE_PRINT_FORMAT = 9;\n"
             f'fprintf ("{ancp}", CLEAR_FILE, af);\n')
    assert txt.count("LFCompute (lf, LF_DONE_COMPUTE);\n") == 1
    txt = txt.replace("LFCompute (lf, LF_DONE_COMPUTE);\n", tail + "LFCompute (lf, LF_DONE_COMPUTE);\n")
    out = hbl.run_script(txt, tmp, binary=binary, extra_env=env)
    return open(ancp).read(), out


CASES = {"codon": lambda: _case("codon", 8, 40, 11), "nuc": lambda: _case("nuc", 8, 300, 21),
         "codon_cat3": lambda: _case("codon", 8, 40, 11, category=CAT)}


@pytest.mark.parametrize("leaves", [False, True], ids=["internal", "doleaves"])
@pytest.mark.parametrize("which", sorted(CASES))
def test_joint_alignment_matches_reference(which, leaves):
    _need_binaries()
    case = CASES[which]()
    anc_cpu, _ = _run(case, None, None, leaves)
    anc_gpu, out = _run(case, HIP_BIN, JENV, leaves)
    assert _joint_calls(out) == 1, out[-600:]            # one partition: exactly one call answered on the device
    assert _device_calls(out) > 0, out[-600:]
    assert len(anc_cpu) > 100 and anc_gpu == anc_cpu


def test_switch_off_runs_the_host_loop():
    _need_binaries()
    case = CASES["codon"]()
    anc_cpu, _ = _run(case, None, None)
    anc_off, out = _run(case, HIP_BIN, OFF)
    assert _joint_calls(out) == 0 and anc_off == anc_cpu


def test_joint_after_optimize_uses_device_matrices():
    """After Optimize the matrices come from the device's exponentials.  The alignment must equal the unmodified reference's over its
    own fit.  The margins recorded in tests/golden/joint_codon_small.npz are those of the given parameters and cannot cover the fit
    Optimize reaches, so the alignment is also compared with the device's own run at HYPHY_HIP_JOINT=0 (the host loop over the host's
    matrices of the same fit)."""
    _need_binaries()
    case = CASES["codon"]()
    anc_cpu, _ = _run(case, None, None, optimize=True)
    anc_off, out_off = _run(case, HIP_BIN, OFF, optimize=True)
    anc_one, out_one = _run(case, HIP_BIN, JENV, optimize=True)
    assert _joint_calls(out_off) == 0 and _joint_calls(out_one) == 1
    assert re.search(r"(\d+) matrix exponentials moved to the device", out_one)
    assert len(anc_cpu) > 100 and anc_one == anc_off == anc_cpu
