// block_checksum_scope.hpp -- the host code above the C ABI (host_stream.cpp, lz4_frame.cpp) sets an engine's block
// checksum switch from its own configuration for the duration of a call, and puts back what the engine's owner set.
#pragma once

#include "engine.hpp"

struct BlockChecksumScope {
    mi355lz4_ctx *c;
    int saved;
    BlockChecksumScope(mi355lz4_ctx *ctx, bool on) : c(ctx), saved(mi355lz4_detail::engine_block_checksum(ctx)) { mi355lz4_set_block_checksum(c, on ? 1 : 0); }
    ~BlockChecksumScope() { mi355lz4_set_block_checksum(c, saved); }
    BlockChecksumScope(const BlockChecksumScope &) = delete;
    BlockChecksumScope &operator=(const BlockChecksumScope &) = delete;
};
