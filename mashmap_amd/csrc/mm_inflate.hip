// mashmap_amd/csrc/mm_inflate.hip -- mm_inflate_blocks: BGZF blocks (independent raw-deflate streams of at most 64 KiB either way)
// inflated on the device, a wave per block.  The decoder is mm_inflate_core.h, the text tests/hostlogic/inflate_check.cpp runs against
// zlib on the host; this file supplies its emission policy for a wave, the kernel around it and the entry points.
#include "mm_internal.h"
#include <algorithm>
#include "mm_inflate_core.h"

static_assert(MM_INFLATE_OK == MMI_OK && MM_INFLATE_BAD_STREAM == MMI_BAD_STREAM && MM_INFLATE_TRUNCATED == MMI_TRUNCATED && MM_INFLATE_OVERRUN == MMI_OVERRUN &&
              MM_INFLATE_SHORT == MMI_SHORT && MM_INFLATE_BAD_DISTANCE == MMI_BAD_DISTANCE && MM_INFLATE_BAD_CRC == MMI_BAD_CRC, "mm_inflate_core.h restates the status values");
static_assert(sizeof(mm_inflate_block) == 32, "mm_inflate_block is 32 bytes");

#define MM_INF_WAVES 4                       // waves per workgroup: 4 x 4.1 KB of tables + 1 KB CRC table + 256 B of literals = 18.2 KB of LDS

// The wave's emission policy.  The 64 lanes run the decoder in lockstep on the same bits (every value it computes is wave-uniform: the
// symbol decode costs what it costs one lane), so literal() and match() are reached by the whole wave at once:
//   * literals are gathered, 64 to a store: every lane writes the byte into the wave's LDS line (the same value to the same address),
//     and a full line -- or whatever is there when a match or the end comes -- leaves as one store instruction, a byte per lane;
//   * a match is copied by the whole wave, byte i from out[pos - distance + i mod distance]: all its source bytes lie before pos, so the
//     lanes are independent of one another also where distance < length (the periodic pattern).
// The output goes to the block's place in the staging buffer in HBM and matches read it back from there.  Producer and consumer are
// lanes of one wave on one CU: the stores must have been performed before the loads are issued, which a workgroup-scope fence
// (__threadfence_block: s_waitcnt vmcnt(0) here, and a barrier for the compiler) orders -- required, because the bytes a match reads
// may have been stored by OTHER lanes of the wave an instruction ago, and sufficient, because a CU's vector L1 is write-through and
// serves the CU's own stores; no other CU ever reads or writes this block's bytes while the kernel runs.
struct MmWaveEmit {
  static constexpr uint32_t kLanes = 64;
  uint8_t* out; uint8_t* lit; uint32_t pos, nLit, ln;
  __device__ uint32_t lane() const { return ln; }
  __device__ void sync() { __threadfence_block(); }                 // the wave's LDS (table) writes before its reads: lgkmcnt(0), in order for the compiler
  __device__ void count(uint32_t* p) { atomicAdd(p, 1u); }
  __device__ void flush() {
    if (!nLit) return;
    if (ln < nLit) out[pos + ln] = lit[ln];                         // (each lane wrote every byte of the line itself: no fence needed to read its own)
    pos += nLit; nLit = 0;
  }
  __device__ void literal(uint8_t b) { lit[nLit] = b; if (++nLit == 64) flush(); }
  __device__ void stored(const uint8_t* src, uint32_t n) {          // a stored block's bytes: copied by the whole wave, 64 to a store
    flush();
    for (uint32_t i = ln; i < n; i += 64) out[pos + i] = src[i];
    pos += n;
  }
  __device__ void match(uint32_t len, uint32_t dist) {
    flush();
    __threadfence_block();                                          // every earlier store of the wave is performed: the loads below may name any of them
    const uint8_t* src = out + pos - dist;
    for (uint32_t i = ln; i < len; i += 64) out[pos + i] = src[i % dist];
    pos += len;
  }
};

// Persistent grid: a wave takes block after block from *next.  status[b] = MM_INFLATE_*; stats: blocks, payload bytes of OK blocks, bad blocks.
// Bounds: the decoder reads comp only inside [cOff, cOff + cLen) and hands the policy only emissions inside [0, uLen) (mm_inflate_core.h);
// the host has checked every descriptor's ranges against the two buffers before the launch.
__global__ __launch_bounds__(64 * MM_INF_WAVES) void k_inflate_blocks(const uint8_t* __restrict__ comp, const mm_inflate_block* __restrict__ desc, uint32_t nBlocks,
                                                                        uint8_t* out, uint32_t* __restrict__ status, unsigned int* next, unsigned long long* stats) {
  __shared__ MmInflateTables tabs[MM_INF_WAVES];
  __shared__ uint32_t crcTab[256];
  __shared__ uint8_t lits[MM_INF_WAVES][64];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) crcTab[i] = mm_crc32_table_entry(i);
  __syncthreads();                                                  // the last workgroup barrier: from here on every wave goes its own way
  const uint32_t wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
  for (;;) {
    uint32_t b = 0;
    if (ln == 0) b = atomicAdd(next, 1u);
    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    if (b >= nBlocks) break;
    const uint64_t cOff = desc[b].cOff, uOff = desc[b].uOff;
    const uint32_t cLen = desc[b].cLen, uLen = desc[b].uLen, want = desc[b].crc32;
    MmWaveEmit e{out + uOff, lits[wave], 0, 0, ln};
    int rc = mm_inflate_decode(e, tabs[wave], comp + cOff, cLen, uLen);
    e.flush();
    if (rc == MMI_OK) {
      // CRC-32 in 64 slices, then the pairwise tree of combine steps (mm_crc32_slice: the right-hand side of a step is 1, 2, 4 ... 32
      // whole slices, its x^(8 len) the square of the step before); lane 0 ends up with the block's
      __threadfence_block();
      uint32_t off, len;
      mm_crc32_slice(uLen, ln, off, len);
      uint32_t crc = mm_crc32_update(crcTab, 0, e.out + off, len);
      uint32_t op = mm_crc32_xpow8(uLen / 64);
      for (uint32_t step = 1; step < 64; step <<= 1) {
        const uint32_t right = (uint32_t)__shfl_down((int)crc, step);
        crc = mm_crc32_combine_op(crc, right, op);
        op = mm_crc32_mulmod(op, op);
      }
      crc = (uint32_t)__builtin_amdgcn_readfirstlane((int)crc);
      if (crc != want) rc = MMI_BAD_CRC;
    }
    if (ln == 0) {
      status[b] = (uint32_t)rc;
      atomicAdd(&stats[0], 1ull);
      if (rc == MMI_OK) atomicAdd(&stats[1], (unsigned long long)uLen); else atomicAdd(&stats[2], 1ull);
    }
    e.sync();                                                       // the tables are the next block's
  }
}

// The error text of a failed mm_inflate_blocks belongs to the thread that made the call: a reader thread may fail here while the
// context's own thread writes mm_ctx::err inside another call, so this path never touches that string.  mm_last_error, called on the
// same thread for the same context, hands the text out once (mm_inflate_take_error) and then answers from mm_ctx::err again.
static thread_local std::string t_inflateErr;
static thread_local const mm_ctx* t_inflateErrCtx = nullptr;
const char* mm_inflate_take_error(const mm_ctx* c) {
  if (!c || t_inflateErrCtx != c) return nullptr;
  t_inflateErrCtx = nullptr;
  return t_inflateErr.c_str();
}
void mm_inflate_keep_error(const mm_ctx* c, InflateErr& e, int rc) {
  if (rc != MM_OK) { t_inflateErr.swap(e.err); t_inflateErrCtx = c; } else if (t_inflateErrCtx == c) t_inflateErrCtx = nullptr;
}

// mm_inflate_blocks (devOut == null: the payloads go to dInfOut and from there to dst) and mm_text_append_inflated (mm_text.hip: they are
// laid end to end at devOut, which holds the sum of the uLen, and stay there; dst is null and nDst SIZE_MAX).  DeviceInput::inflateMu is held.
int mm_inflate_run(mm_ctx* c, InflateErr* e, const void* comp, size_t nComp, mm_inflate_block* blocks, size_t nBlocks, void* dst, size_t nDst, size_t* nBad, uint8_t* devOut) {
  DeviceInput::Inflate& I = c->input.inf;
  if (nBlocks && (!blocks || !comp || (!dst && nDst && !devOut))) { e->err = "mm_inflate_blocks: null argument"; return MM_ERR_ARG; }
  if (nBlocks > 0x7fffffffu) { e->err = "mm_inflate_blocks: too many blocks"; return MM_ERR_ARG; }
  // every range inside its buffer, no two output ranges overlapping; nothing is launched before this has passed
  uint64_t cLo = ~0ull, cHi = 0;
  I.infOrder.clear();
  for (size_t i = 0; i < nBlocks; i++) {
    const mm_inflate_block& b = blocks[i];
    if (b.cLen > MM_INFLATE_MAX_BLOCK || b.uLen > MM_INFLATE_MAX_BLOCK) { e->err = "mm_inflate_blocks: a block above MM_INFLATE_MAX_BLOCK"; return MM_ERR_ARG; }
    if (b.cOff > nComp || nComp - b.cOff < b.cLen || b.uOff > nDst || nDst - b.uOff < b.uLen) { e->err = "mm_inflate_blocks: a descriptor's range leaves its buffer"; return MM_ERR_ARG; }
    if (b.cLen) { cLo = std::min<uint64_t>(cLo, b.cOff); cHi = std::max<uint64_t>(cHi, b.cOff + b.cLen); }
    if (b.uLen) I.infOrder.push_back((uint32_t)i);
  }
  std::sort(I.infOrder.begin(), I.infOrder.end(), [&](uint32_t a, uint32_t b) { return blocks[a].uOff < blocks[b].uOff; });
  for (size_t k = 1; k < I.infOrder.size(); k++) {
    const mm_inflate_block& p = blocks[I.infOrder[k - 1]];
    if (p.uOff + p.uLen > blocks[I.infOrder[k]].uOff) { e->err = "mm_inflate_blocks: output ranges overlap"; return MM_ERR_ARG; }
  }
  if (!nBlocks) { I.infCalls++; return MM_OK; }
  if (cLo > cHi) cLo = cHi = 0;

  { const int rc = c->input.ready(c->device, e); if (rc != MM_OK) return rc; }
  MM_HIP(e, I.infEvA.ensure());
  MM_HIP(e, I.infEvB.ensure());
  hipStream_t st = c->input.inflateStream;
  // device descriptors: cOff relative to the compressed span, payloads packed end to end in ascending uOff (what is adjacent in dst stays
  // adjacent on the device, so a run of adjacent ranges comes back as one copy)
  I.infDesc.assign(blocks, blocks + nBlocks);
  uint64_t at = 0;
  for (uint32_t i : I.infOrder) { I.infDesc[i].uOff = at; at += blocks[i].uLen; }
  for (size_t i = 0; i < nBlocks; i++) { if (!blocks[i].uLen) I.infDesc[i].uOff = 0; I.infDesc[i].cOff = blocks[i].cLen ? blocks[i].cOff - cLo : 0; I.infDesc[i].status = 0; }
  MM_HIP(e, I.dInfComp.ensure((size_t)(cHi - cLo) + 64));
  if (!devOut) MM_HIP(e, I.dInfOut.ensure((size_t)at + 64));
  MM_HIP(e, I.dInfDesc.ensure(nBlocks * sizeof(mm_inflate_block)));
  MM_HIP(e, I.dInfStatus.ensure(nBlocks * sizeof(uint32_t)));
  if (!I.dInfStats.p) { MM_HIP(e, I.dInfStats.ensure(64)); MM_HIP(e, hipMemsetAsync(I.dInfStats.p, 0, 64, st)); }
  if (!I.infGrid) {
    int cus = 0, perCu = 0;
    MM_HIP(e, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    MM_HIP(e, hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, k_inflate_blocks, 64 * MM_INF_WAVES, 0));
    I.infGrid = std::max(1, cus) * std::max(1, perCu);         // what the device holds at the kernel's residency
  }
  if (cHi > cLo) MM_HIP(e, hipMemcpyAsync(I.dInfComp.p, (const char*)comp + cLo, (size_t)(cHi - cLo), hipMemcpyHostToDevice, st));
  MM_HIP(e, hipMemcpyAsync(I.dInfDesc.p, I.infDesc.data(), nBlocks * sizeof(mm_inflate_block), hipMemcpyHostToDevice, st));
  MM_HIP(e, hipMemsetAsync(I.dInfStats.p, 0, 8, st));                       // the block counter starts over; the three counts behind it go on
  unsigned long long* stats = I.dInfStats.as<unsigned long long>();
  const unsigned grid = (unsigned)std::min<size_t>((size_t)I.infGrid, (nBlocks + MM_INF_WAVES - 1) / MM_INF_WAVES);
  MM_HIP(e, hipEventRecord(I.infEvA, st));
  hipLaunchKernelGGL(k_inflate_blocks, dim3(grid), dim3(64 * MM_INF_WAVES), 0, st, I.dInfComp.as<uint8_t>(), I.dInfDesc.as<mm_inflate_block>(), (uint32_t)nBlocks,
                     devOut ? devOut : I.dInfOut.as<uint8_t>(), I.dInfStatus.as<uint32_t>(), (unsigned int*)stats, stats + 1);
  MM_HIP(e, hipGetLastError());
  MM_HIP(e, hipEventRecord(I.infEvB, st));
  // the payloads back, one copy per run of adjacent output ranges
  for (size_t k = 0; !devOut && k < I.infOrder.size();) {
    size_t j = k + 1;
    while (j < I.infOrder.size() && blocks[I.infOrder[j - 1]].uOff + blocks[I.infOrder[j - 1]].uLen == blocks[I.infOrder[j]].uOff) j++;
    const mm_inflate_block& first = blocks[I.infOrder[k]]; const mm_inflate_block& last = blocks[I.infOrder[j - 1]];
    MM_HIP(e, hipMemcpyAsync((char*)dst + first.uOff, I.dInfOut.as<char>() + I.infDesc[I.infOrder[k]].uOff, (size_t)(last.uOff + last.uLen - first.uOff), hipMemcpyDeviceToHost, st));
    k = j;
  }
  I.infStatus.resize(nBlocks);
  uint64_t hStats[4] = {0, 0, 0, 0};
  MM_HIP(e, hipMemcpyAsync(I.infStatus.data(), I.dInfStatus.p, nBlocks * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MM_HIP(e, hipMemcpyAsync(hStats, I.dInfStats.p, sizeof hStats, hipMemcpyDeviceToHost, st));
  MM_HIP(e, hipStreamSynchronize(st));
  I.infCalls++;                                                  // a call that ran: counted behind its one wait
  size_t bad = 0;
  for (size_t i = 0; i < nBlocks; i++) { blocks[i].status = I.infStatus[i]; bad += I.infStatus[i] != MM_INFLATE_OK; }
  if (nBad) *nBad = bad;
  I.infBlocks = hStats[1]; I.infBytes = hStats[2]; I.infBad = hStats[3];
  float ms = 0;
  if (hipEventElapsedTime(&ms, I.infEvA, I.infEvB) == hipSuccess) I.infKernelMs = ms; else (void)hipGetLastError();
  return MM_OK;
}

extern "C" {

int mm_inflate_blocks(mm_ctx* c, const void* comp, size_t nComp, mm_inflate_block* blocks, size_t nBlocks, void* dst, size_t nDst, size_t* nBad) {
  if (nBad) *nBad = 0;
  return mm_input_call(c, [&](InflateErr* e) { return mm_inflate_run(c, e, comp, nComp, blocks, nBlocks, dst, nDst, nBad, nullptr); });
}

int mm_inflate_counts(const mm_ctx* c, uint64_t* calls, uint64_t* blocks, uint64_t* bytesOut) {
  if (!c) return MM_ERR_ARG;
  std::lock_guard<std::mutex> lock(c->input.inflateMu);
  if (calls) *calls = c->input.inf.infCalls;
  if (blocks) *blocks = c->input.inf.infBlocks;
  if (bytesOut) *bytesOut = c->input.inf.infBytes;
  return MM_OK;
}

int mm_inflate_kernel_ms(const mm_ctx* c, double* ms) {
  if (!c || !ms) return MM_ERR_ARG;
  std::lock_guard<std::mutex> lock(c->input.inflateMu);
  *ms = c->input.inf.infKernelMs;
  return MM_OK;
}

}  // extern "C"
