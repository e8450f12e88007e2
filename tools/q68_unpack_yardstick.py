"""Yardstick for the code caps of tests/test_cache_q68.py::test_q68_cache_decodes_on_the_chain: the same cases on the module-by-module
UNPACK route (EXL2_Q4_FUSED=0, EXL2_CHAIN=0 -- q_to_fp16_kv + fp16 attention + fp16_to_q_kv, the kernels that are bit-exact against the
reference's), emulation build.  Prints, per side width, the worst fraction of the step's own token's codes that differ from the
oracle's, the largest code difference and the worst scale distance in fp16 ulp.  The test's cap for 8-bit sides is twice the worst.

    python tools/q68_unpack_yardstick.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["EXL2_Q4_FUSED"] = "0"
os.environ.setdefault("EXL2_ENV_DYNAMIC", "1")

import pytest  # noqa: E402
from tests import conftest, test_cache_q68 as T  # noqa: E402


def main():
    be = conftest.Backend("emu")
    mp = pytest.MonkeyPatch()
    worst = {}
    try:
        for wbits in (6, 8):
            for recipe, batch, hd, _ in T.CHAIN_CASES:
                stats = []
                T._q68_chain_case(be, mp, T._chain_cfg(hd), wbits, recipe, batch, 6, chains=("0",), stats=stats)
                for bits, frac, code, ulp in stats:
                    w = worst.setdefault((wbits, bits), [0.0, 0, 0])
                    w[0], w[1], w[2] = max(w[0], frac), max(w[1], code), max(w[2], ulp)
                print(wbits, recipe, batch, hd, {b: round(max(f for bb, f, _, _ in stats if bb == b), 5) for b in {s[0] for s in stats}}, flush=True)
    finally:
        mp.undo()
    for (wbits, bits), (frac, code, ulp) in sorted(worst.items()):
        print(f"Q{wbits} {bits}-bit side: worst new-token code fraction {frac:.5f}, largest code difference {code}, worst scale ulp {ulp}")


if __name__ == "__main__":
    main()
