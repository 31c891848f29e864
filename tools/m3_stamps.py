"""Reads the s_memrealtime stamps of a -DVAEK_M3_STAMPS build of libvaek.so (VAEK_LIB_PATH; tools/m3_stamps.sh builds it)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from vae_training_amd.engine import Engine  # noqa: E402

B, D, L = 100, 6, 6
eng = Engine(B, D, L, (200, 200, 200), (200, 200, 200), -3.0, True, False)
assert eng.step_path == "mlp3"
torch.manual_seed(0)
params = torch.randn(eng.P, device="cuda") * 0.1
grads = eng.new_flat(eng.grad_len); m = eng.new_flat(); v = eng.new_flat()
step = torch.zeros(1, dtype=torch.int32, device="cuda")
x, z1, z2 = torch.randn(B, D, device="cuda"), torch.randn(B, L, device="cuda"), torch.randn(B, D, device="cuda")
buf = torch.zeros(32, dtype=torch.int64, device="cuda")
eng.lib.vaek_debug_set_stamps.argtypes = [C.c_void_p, C.c_void_p]
assert eng.lib.vaek_debug_set_stamps(eng.h, C.c_void_p(buf.data_ptr())) == 0
for _ in range(6):
    eng.train_step(params, grads, m, v, step, x, z1, z2, 1e-4)
torch.cuda.synchronize()
t = buf.cpu().numpy()
names = (["inputs -> LDS, small vectors"] + [f"forward layer {i} ({'encoder' if i < 4 else 'decoder'})" + (" + reparam" if i == 3 else "") for i in range(8)]
         + ["ELBO elementwise"] + [f"dX of layer {i}" + (" + reparam backward" if i == 4 else "") for i in range(7, 0, -1)] + ["partial row"])
print("workgroup 0 of fused_mlp3_chain (us, s_memrealtime at 100 MHz; each stamp drains the wave's memory operations first):")
for i, n in enumerate(names):
    print(f"   {n:40s} {(t[i + 1] - t[i]) / 100.0:7.2f}")
print(f"   total {(t[18] - t[0]) / 100.0:.2f}")
