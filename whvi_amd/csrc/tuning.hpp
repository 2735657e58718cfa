#pragma once
// whvi_amd/csrc/tuning.hpp -- every switch that exists for MEASUREMENTS only, in one place.
//
// The shipped library (whvi_amd/csrc/Makefile never defines WHVI_TUNING_BUILD) contains none of them: no getenv, no
// alternative instruction forms, no trace hooks -- its launch form depends on its arguments alone
// (tests/test_abi.py::test_shipped_library_reads_no_environment).  Probe builds (`make -C whvi_amd/csrc tuning
// [DEFS=-D...]` -> whvi_amd/_exp/libwhvi_hip_tuning.so, loaded by tools/ through WHVI_HIP_LIB) define it and get
//   * WHVI_TUNE_ENV(name): environment A/B switches of the dispatch (read once per process), DESIGN.md 6.3;
//   * the -D overrides below, some of which produce WRONG VALUES on purpose (timing-only instruction swaps).
#ifdef WHVI_TUNING_BUILD
#include <stdlib.h>
#define WHVI_TUNE_ENV(name) getenv(name)
#else
#define WHVI_TUNE_ENV(name) ((const char *)nullptr)
#if defined(WHVI_F16_UNPACK) || defined(WHVI_F16_PACK_EXP) || defined(WHVI_BF16_PACK) || defined(WHVI_NO_PK) || \
    defined(WHVI_BLOCK_TRACE) || defined(WHVI_ROWS_STORE_FORM) || defined(WHVI_ALIGN_SINGLE_PASS)
#error "kernel tuning switches need -DWHVI_TUNING_BUILD (make -C whvi_amd/csrc tuning DEFS=-D...)"
#endif
#endif

// ---- production values (a tuning build may override them with -D) ------------------------------------------------
// (WHVI_F16_PACK_EXP, WHVI_NO_PK and WHVI_BLOCK_TRACE have no value: they are tested with #ifdef where they act.)
#ifndef WHVI_F16_UNPACK
#define WHVI_F16_UNPACK 1          // fp16 unpack with an explicit shift for the high half (kernels.hpp: Elem<__half>)
#endif
#ifndef WHVI_BF16_PACK
#define WHVI_BF16_PACK 1           // one v_cvt_pk_bf16_f32 per output dword
#endif
#ifndef WHVI_ALIGN_SINGLE_PASS
#define WHVI_ALIGN_SINGLE_PASS -1      // store-barrier launches without the tile loop in the code: -1 = per-type rule (kernels.hpp), -2 = 16-bit storage only, 0 / 1 force
#endif
#ifndef WHVI_ROWS_STORE_FORM
#define WHVI_ROWS_STORE_FORM 0         // streaming stores of the plain transform: 0 = one vector offset per chunk, 1 = scalar offsets (the mutant of tests/test_build.py)
#endif
