// Ring membership on its own (k_member.hip, api_member.hip): the launch wrappers (the ZKM1 layout is in wire.h) of the kernels around the shared GK machinery.
#pragma once
#include "engine.h"
void launch_m_front(hipStream_t s, const Workspace& W, uint32_t count, const uint32_t* which, const uint8_t* blinder, uint64_t first, uint32_t* which_s);
void launch_m_write_head(hipStream_t s, const Workspace& W, uint32_t count, uint64_t first, uint32_t size, uint8_t* out, uint8_t* com, uint8_t* blinder_out, int32_t* status);
void launch_mv_header_validate(hipStream_t s, const VWork& V, uint32_t count, const uint8_t* proofs, const uint64_t* off, uint64_t first);
void launch_mv_offsets(hipStream_t s, uint64_t* off, uint64_t B, uint64_t size);
void launch_mv_final(hipStream_t s, const Workspace& W, const VWork& V, uint32_t count, uint8_t* ok, int32_t* status, uint64_t first);
