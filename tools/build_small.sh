#!/bin/bash
cd "$(dirname "$0")/.." || exit 1
hipcc -O3 -std=c++17 --offload-arch=gfx950 -DBIEM_GEMM_TRACE "$@" tools/gemm_small.cpp \
  biem_helmholtz_sphere_amd/csrc/abi.cpp biem_helmholtz_sphere_amd/csrc/solve_path.cpp biem_helmholtz_sphere_amd/csrc/plan.cpp biem_helmholtz_sphere_amd/csrc/plan_tree.cpp biem_helmholtz_sphere_amd/csrc/plan_fill.cpp biem_helmholtz_sphere_amd/csrc/kernels_tables.hip biem_helmholtz_sphere_amd/csrc/kernels_fill.hip biem_helmholtz_sphere_amd/csrc/kernels_fill_sym.hip biem_helmholtz_sphere_amd/csrc/kernels_rhs.hip \
  biem_helmholtz_sphere_amd/csrc/kernels_uscat.hip biem_helmholtz_sphere_amd/csrc/kernels_uinterior.hip biem_helmholtz_sphere_amd/csrc/kernels_power.hip biem_helmholtz_sphere_amd/csrc/kernels_force.hip \
  biem_helmholtz_sphere_amd/csrc/kernels_gemm3m.hip biem_helmholtz_sphere_amd/csrc/kernels_lu.hip biem_helmholtz_sphere_amd/csrc/kernels_sym.hip biem_helmholtz_sphere_amd/csrc/kernels_trisolve.hip -o tools/gemm_small 2>&1 | grep -v warning | head
