"""Developer tool (GPU): where does RawNet2's 16-bit path leave the fp32 engine?  Options rn_keep + rn_unfused = 1 (the separate kernel
sequence, which stores every stage on both handles): the 16-bit handle's stage against the exact-fp32 handle's for the front-end output
(rn_front) and then the PRE-ACTIVATIONS lrelu(bn(x)) that block n reads after n residual blocks (rn_b<n>_pre, n = 1..7; rn_agg_in after
all eight), then the pooled statistics and the embedding.  No oracle involved: both sides are the library.
python tools/rn_stage_err.py [f16|bf16] [B] [seed_w]"""
import sys
sys.path.insert(0, '.')
import numpy as np
from speakerverification_amd import synth
from speakerverification_amd.engine import Engine

mode = sys.argv[1] if len(sys.argv) > 1 else "f16"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 2
seed_w = int(sys.argv[3]) if len(sys.argv) > 3 else 1
sd = synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320), seed=seed_w)
x = synth.synth_waveforms(B, 32000, seed=20220829)
engs, out, st = {}, {}, {}
for c in ("f32", mode):
    e = Engine(model="rawnet2", compute=c, embed_dim=320, max_batch=B)
    e.load_state_dict(sd)
    e.finalize()
    out[c] = e.embed_wave(x).reshape(B, -1).copy()          # the embedding and the pooled statistics: the forward that ships
    st[c] = e.get_stage("rn_pooled").reshape(B, 2, 512).copy()
    e.set_option("rn_keep", 1)
    e.set_option("rn_unfused", 1)
    e.embed_wave(x)
    engs[c] = e
for n, stage in enumerate(["rn_front"] + [f"rn_b{i}_pre" for i in range(1, 8)] + ["rn_agg_in"]):
    a, b = engs["f32"].get_stage(stage), engs[mode].get_stage(stage)
    print(f"after {n} blocks ({stage}): elements {a.size:9d}  scale {np.abs(a).max():9.3f}  max err / scale {np.abs(a - b).max() / np.abs(a).max():.5f}  "
          f"rms err / rms {np.sqrt(((a - b) ** 2).mean() / (a ** 2).mean()):.5f}")
for k, name in ((0, "weighted mean"), (1, "weighted std")):
    a, b = st["f32"][:, k], st[mode][:, k]
    print(f"{name}: scale {np.abs(a).max():.3f}  max err / scale {np.abs(a - b).max() / np.abs(a).max():.5f}")
a, b = out["f32"], out[mode]
cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
print(f"embedding ({mode} vs f32): cos {cos}  max err / scale {np.abs(a - b).max() / np.abs(a).max():.5f}")
