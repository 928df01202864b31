"""Developer tool (CPU): print the bars of tests/conformer_oracle_check.py — 3 x the clean emulation's worst error of every check, per
compute, over the lengths the GPU file runs — in the form the module holds them.  Run from the repository root:

    python tools/conformer_oracle_bars.py

The GPU's worst values (third column of the module's tables) come from tests/test_gpu_conformer_oracle.py's printed output."""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import conformer_oracle_check as chk  # noqa: E402


def bar_of(e):
    """3 x the emulation's value (as printed, two significant digits), rounded up to two significant digits"""
    x = 3 * float(f"{e:.1e}")
    p = math.floor(math.log10(x)) - 1
    return math.ceil(x / 10 ** p - 1e-9) * 10 ** p


def main():
    for compute in ("f32", "bf16"):
        worst = chk.emulation_worst(compute)
        print(f"{compute.upper()}_BARS = {{")
        for n in chk.CHECKS:
            print(f'    "{n}": {bar_of(worst[n]):.1e},'.ljust(32) + f"# {worst[n]:.1e}")
        print("}")


if __name__ == "__main__":
    main()
