"""Developer tool (CPU): print the bars of tests/resnetse_oracle_check.py — 3 x the clean emulation's worst error of every check, per
compute, over the cases the GPU file runs (edge lengths, the n_mels = 64, 'SAP' and no-log configurations, the ragged packs, full size
from waveforms) — in the form the module holds them.  Run from the repository root:

    python tools/resnetse_oracle_bars.py

The GPU's worst values (third column of the module's tables) come from tests/test_gpu_resnetse_oracle.py's printed output."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import resnetse_oracle_check as chk  # noqa: E402


def main():
    for compute in ("f32", "bf16"):
        worst = chk.emulation_worst(compute)
        print(f"{compute.upper()}_BARS = {{")
        for n in chk.CHECKS:
            print(f'    "{n}": {3 * worst[n]:.1e},'.ljust(36) + f"# {worst[n]:.1e},")
        print("}")


if __name__ == "__main__":
    main()
