// fxg_stub_ctx.h -- TEST-ONLY: the context of the emulation stub (fxg_stub.cpp), for the units that put more entry points behind it (bcsplit_stub.cpp)
#pragma once
#include "../../include/fxg.h"
struct fxg_emu_hist;
struct fxg_ctx { char err[512]; uint64_t scratch[FXG_NCOUNTERS]; fxg_emu_hist *hist; uint64_t text_state[16]; int device; };
