# Diagnostic builds (-DVAEK_M3_STAMPS): where workgroup 0 of the three-hidden-layer chain kernel (csrc/fused_mlp3.hip) spends its
# time, on line 1 of sphere_vae_padding_expts.sh (200|200|200, D = 6, L = 6, batch 100) -- first as shipped, then with
# -DVAEK_M3_NO_VEC (dX with dword loads instead of 16-byte ones).  profiles/mlp3_stamps.txt is this script's output.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
B=${M3_BUILD_DIR:-/tmp/m3st}
cd $R/vae_training_amd/csrc
mkdir -p $B $B/nv
ls *.hip | sed "s/\.hip$//" | xargs -P 8 -I{} /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -DVAEK_M3_STAMPS -c {}.hip -o $B/{}.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $B/libvaek.so $B/*.o
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -DVAEK_M3_STAMPS -DVAEK_M3_NO_VEC -c fused_mlp3.hip -o $B/nv/fused_mlp3.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $B/nv/libvaek.so $(ls $B/*.o | grep -v fused_mlp3.o) $B/nv/fused_mlp3.o
cd $R
echo "== as shipped (dX: 16-byte loads along k)"
VAEK_LIB_PATH=$B/libvaek.so timeout -k 10 120 python3 tools/m3_stamps.py
echo "== -DVAEK_M3_NO_VEC (dX: dword loads)"
VAEK_LIB_PATH=$B/nv/libvaek.so timeout -k 10 120 python3 tools/m3_stamps.py
