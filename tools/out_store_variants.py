#!/usr/bin/env python
"""DEVELOPMENT: builds libpfamd_os{1,2,3}.so - the float scalar-state VEC = 4 step kernels (both tile geometries) with the
output stores non-temporal / sc1 / sc0 sc1 (pf_device.hpp: PF_OUT_STORE), everything else from build/obj - for
    PF_AMD_LIB=pyfilter_amd/libpfamd_os2.so python tools/kbench.py apf_lgo_1m ..."""
from build_some import rebuild

for k in (1, 2, 3):
    print(rebuild(["f32d1_v4_m0", "f32d1_v4_m1"], [f"-DPF_OUT_STORE={k}"], f"os{k}"))
