#!/bin/bash
# builds the diagnostic tool tools/gemm_trace<suffix> (see tools/gemm_trace.cpp); usage: build_trace.sh [suffix] [extra hipcc flags...]
# flags: -DBIEM_TR_STAMPS (in-kernel timeline; perturbs) and the timing ablations -DBIEM_ABL_{NOMFMA,NODMA,NOCDMA,ONLYCDMA,NOLDS,NOSUMS,NOCADD,
# NOBARRIER,NOEPI,NOSTORE,ONESTORE,CHOT} (results wrong by construction, only the launch time is meaningful).
# NOLDS, NOCDMA, ONLYCDMA and CHOT redefine a piece of the chunk loop's asm statement (kernels_gemm3m.hip, above gemm3m_body), so they act
# on every kernel instance whose statements use that piece, not on the K = 128 / 256 form alone; NDMA follows them
cd "$(dirname "$0")/.." || exit 1
suf="$1"; shift
hipcc -O3 -std=c++17 --offload-arch=gfx950 -DBIEM_GEMM_TRACE "$@" tools/gemm_trace.cpp \
  biem_helmholtz_sphere_amd/csrc/*.cpp biem_helmholtz_sphere_amd/csrc/*.hip -o tools/gemm_trace$suf 2>/dev/null
