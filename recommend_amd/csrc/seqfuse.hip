// Timestamp-aware sequence fusion (include/onetrans_hip.h, "sequence fusion"): the row map that interleaves a
// sample's behaviour events by time.  Per sample the L_S events of its nseq sequences are ordered by the key
//   (time, index of the sequence among the descriptors, position in the sequence)
// which is a total order, so the ranks are a permutation of 0 .. L_S-1 whatever the times are (unsorted
// sequences, ties, all equal).  Event j of sequence i in sample b gets
//   out_rows[map_off_i + b * L_i + j] = b * row_stride + rank
// the output-row entry of the per-sequence projection GEMM's row map: the GEMM then scatters every projected
// event straight to its place in the time-ordered token stream.
//
// One workgroup per sample.  The keys sit in LDS as the time with its sign bit flipped (unsigned order = signed
// order) plus a 32-bit tag, the event's index in the concatenation of the sequences (ascending in (sequence,
// position)); a bitonic network over the next power of two P >= L_S sorts the (key, tag) pairs, the padding
// slots holding the largest pair.  12 bytes per slot: 48 KiB at the limit L_S = 4096.  The workgroup has
// min(256, max(64, P / 2)) threads, so a short stream (C2: 126 events) is sorted by a single wave.
#include "common.h"

namespace ot {

constexpr int SEQFUSE_MAX_L = 4096;
constexpr int SEQFUSE_MAX_SEQ = 32;
constexpr uint64_t SEQFUSE_SIGN = 0x8000000000000000ull;

struct SeqFuseArgs {                     // the descriptors, by value (validated on the host)
  const int64_t* times[SEQFUSE_MAX_SEQ];
  int64_t stride_b[SEQFUSE_MAX_SEQ];
  int32_t map_off[SEQFUSE_MAX_SEQ];
  int32_t start[SEQFUSE_MAX_SEQ + 1];    // first concatenation index of each sequence; start[nseq] = L_S
};

// the sequence holding concatenation index c (start ascending, start[0] = 0 <= c < start[nseq]); empty sequences
// are skipped because the last start <= c wins
__device__ __forceinline__ int seqfuse_owner(const int32_t* start, int nseq, int c) {
  int i = 0;
  for (int k = 1; k < nseq; ++k)
    if (start[k] <= c) i = k;
  return i;
}

__global__ __launch_bounds__(256) void seq_time_rows_kernel(SeqFuseArgs a, int nseq, int L_S, int P,
                                                            int64_t row_stride, int32_t* __restrict__ out_rows,
                                                            int32_t* __restrict__ rank_out,
                                                            int64_t* __restrict__ last_time) {
  extern __shared__ uint64_t seqfuse_lds[];
  uint64_t* keys = seqfuse_lds;                     // [P]
  uint32_t* tags = (uint32_t*)(seqfuse_lds + P);    // [P]
  __shared__ int32_t start[SEQFUSE_MAX_SEQ + 1];
  __shared__ int32_t map_off[SEQFUSE_MAX_SEQ];
  __shared__ const int64_t* times[SEQFUSE_MAX_SEQ];
  __shared__ int64_t stride_b[SEQFUSE_MAX_SEQ];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (tid <= nseq) start[tid] = a.start[tid];       // (at least 64 threads, at most 33 entries)
  if (tid < nseq) {
    map_off[tid] = a.map_off[tid];
    times[tid] = a.times[tid];
    stride_b[tid] = a.stride_b[tid];
  }
  __syncthreads();
  for (int c = tid; c < P; c += nt) {
    if (c < L_S) {
      const int i = seqfuse_owner(start, nseq, c);
      const int64_t t = times[i][(int64_t)b * stride_b[i] + (c - start[i])];
      keys[c] = (uint64_t)t ^ SEQFUSE_SIGN;
      tags[c] = (uint32_t)c;
    } else {
      keys[c] = ~0ull;                              // padding: above every event (a real tag is < 2^32 - 1)
      tags[c] = 0xFFFFFFFFu;
    }
  }
  // bitonic sort, ascending in (key, tag)
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (P >> 1); t += nt) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool asc = (i & size) == 0;
        const uint64_t ki = keys[i], kj = keys[j];
        const uint32_t ti = tags[i], tj = tags[j];
        const bool gt = ki > kj || (ki == kj && ti > tj);
        if (gt == asc) {                            // pairs are distinct: !gt is "less"
          keys[i] = kj; keys[j] = ki;
          tags[i] = tj; tags[j] = ti;
        }
      }
    }
  }
  __syncthreads();
  for (int r = tid; r < L_S; r += nt) {
    const int c = (int)tags[r];
    const int i = seqfuse_owner(start, nseq, c);
    const int L = start[i + 1] - start[i];
    out_rows[(int64_t)map_off[i] + (int64_t)b * L + (c - start[i])] = (int32_t)((int64_t)b * row_stride + r);
    if (rank_out) rank_out[(int64_t)b * L_S + c] = r;
  }
  if (tid == 0 && last_time) last_time[b] = (int64_t)(keys[L_S - 1] ^ SEQFUSE_SIGN);
}

}  // namespace ot

using namespace ot;

// The sort lives in LDS: no scratch memory is used.  One 256-byte unit is asked for so that the call keeps the
// library's (workspace, ws_bytes) form and a later path above the LDS limit can grow it.
extern "C" size_t ot_seq_time_rows_workspace_size(int B, int nseq, int L_S) {
  if (B < 0 || nseq < 1 || nseq > SEQFUSE_MAX_SEQ || L_S < 1 || L_S > SEQFUSE_MAX_L) return 0;
  return 256;
}

extern "C" int ot_seq_time_rows(const ot_seq_time* seqs, int nseq, int B, int L_S, int64_t row_stride,
                                int32_t* out_rows, int32_t* rank_out, int64_t* last_time, void* workspace,
                                size_t ws_bytes, void* stream) {
  OT_REQUIRE(nseq >= 1 && nseq <= SEQFUSE_MAX_SEQ, "ot_seq_time_rows: nseq=%d out of range (1..%d)", nseq,
             SEQFUSE_MAX_SEQ);
  OT_REQUIRE(B >= 0, "ot_seq_time_rows: B=%d is negative", B);
  OT_REQUIRE(L_S >= 1 && L_S <= SEQFUSE_MAX_L, "ot_seq_time_rows: L_S=%d unsupported (1..%d)", L_S, SEQFUSE_MAX_L);
  OT_REQUIRE(row_stride >= L_S, "ot_seq_time_rows: row_stride < L_S");
  OT_REQUIRE((int64_t)B * row_stride <= (int64_t)INT32_MAX, "ot_seq_time_rows: B * row_stride exceeds int32 rows");
  const size_t need = ot_seq_time_rows_workspace_size(B, nseq, L_S);
  OT_REQUIRE(ws_bytes >= need, "ot_seq_time_rows: workspace too small (%zu < %zu)", ws_bytes, need);
  OT_REQUIRE(seqs, "ot_seq_time_rows: null descriptors");
  SeqFuseArgs a{};
  int64_t total = 0;
  for (int i = 0; i < nseq; ++i) {
    const ot_seq_time& q = seqs[i];
    OT_REQUIRE(q.L >= 0 && q.map_off >= 0, "ot_seq_time_rows: sequence %d: negative L or map_off", i);
    OT_REQUIRE(q.stride_b >= q.L, "ot_seq_time_rows: sequence %d: stride_b < L", i);
    OT_REQUIRE((int64_t)q.map_off + (int64_t)B * q.L <= (int64_t)INT32_MAX,
               "ot_seq_time_rows: sequence %d: map segment exceeds int32", i);
    OT_REQUIRE(B == 0 || q.L == 0 || q.times, "ot_seq_time_rows: sequence %d: null times", i);
    a.times[i] = q.times;
    a.stride_b[i] = q.stride_b;
    a.map_off[i] = q.map_off;
    a.start[i] = (int32_t)total;
    total += q.L;
    OT_REQUIRE(total <= L_S, "ot_seq_time_rows: the sequences hold more than L_S=%d events", L_S);
  }
  OT_REQUIRE(total == L_S, "ot_seq_time_rows: the sequences hold %lld events, L_S=%d", (long long)total, L_S);
  a.start[nseq] = (int32_t)total;
  if (B == 0) return OT_OK;
  OT_REQUIRE(out_rows && workspace, "ot_seq_time_rows: null operand");
  int P = 1;
  while (P < L_S) P <<= 1;
  const int threads = P / 2 < 64 ? 64 : (P / 2 > 256 ? 256 : P / 2);
  hipLaunchKernelGGL(seq_time_rows_kernel, dim3(B), dim3(threads), (size_t)P * 12, (hipStream_t)stream, a, nseq,
                     L_S, P, row_stride, out_rows, rank_out, last_time);
  OT_LAUNCH_CHECK("ot_seq_time_rows");
  return OT_OK;
}

// ------------------------------------------------------------------------------------------
// Key-padding mask of layer 0 (include/onetrans_hip.h, "padding mask"): valid0[b][p] = 1 for [SEP] and NS tokens;
// event j of sequence i (left-padded: its real events are the last len_i[b]) is valid iff j >= L_i - len_i[b], and
// sits at its concatenation position off_i + j, or under time fusion at its rank in the time order (ot_seq_time_rows'
// rank_out, indexed by the event's index in the concatenation of the sequences) — nothing is assumed about where
// padding sorts.  One thread per (sample, concatenation position): the ranks are a permutation of the event
// positions, so every byte of valid0 has one writer.  Lengths outside [0, L_i] are clamped here.
namespace ot {

struct SeqValidArgs {
  int32_t L[SEQFUSE_MAX_SEQ], off[SEQFUSE_MAX_SEQ], start[SEQFUSE_MAX_SEQ];
};

__global__ __launch_bounds__(256) void seq_key_valid_kernel(SeqValidArgs a, int nseq, const int32_t* __restrict__ lens,
                                                            int B, int L0, const int32_t* __restrict__ rank,
                                                            int64_t ldr, uint8_t* __restrict__ valid0) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)B * L0) return;
  const int b = (int)(e / L0), c = (int)(e % L0);
  int pos = c;
  uint8_t v = 1;
  for (int i = 0; i < nseq; ++i) {
    const int j = c - a.off[i];
    if (j >= 0 && j < a.L[i]) {
      int len = lens[(int64_t)i * B + b];
      len = len < 0 ? 0 : (len > a.L[i] ? a.L[i] : len);
      v = j >= a.L[i] - len;
      if (rank) pos = rank[(int64_t)b * ldr + a.start[i] + j];
      break;
    }
  }
  if ((unsigned)pos < (unsigned)L0) valid0[(int64_t)b * L0 + pos] = v;   // (a rank outside the row is not written)
}

}  // namespace ot

extern "C" int ot_seq_key_valid(const int32_t* lens, const int32_t* seq_len, const int32_t* seq_off, int nseq, int B,
                                int L0, const int32_t* rank, int64_t ldr, uint8_t* valid0, void* stream) {
  OT_REQUIRE(nseq >= 0 && nseq <= SEQFUSE_MAX_SEQ, "ot_seq_key_valid: nseq=%d out of range (0..%d)", nseq,
             SEQFUSE_MAX_SEQ);
  OT_REQUIRE(B >= 0 && L0 >= 1, "ot_seq_key_valid: bad sizes B=%d L0=%d", B, L0);
  OT_REQUIRE(nseq == 0 || (seq_len && seq_off), "ot_seq_key_valid: null descriptors");
  SeqValidArgs a{};
  int64_t total = 0;
  int prev_end = 0;
  for (int i = 0; i < nseq; ++i) {
    OT_REQUIRE(seq_len[i] >= 0 && seq_off[i] >= prev_end && (int64_t)seq_off[i] + seq_len[i] <= L0,
               "ot_seq_key_valid: sequence %d: segment [%d, %d) overlaps its predecessor or leaves the %d tokens", i,
               seq_off[i], seq_off[i] + seq_len[i], L0);
    a.L[i] = seq_len[i];
    a.off[i] = seq_off[i];
    a.start[i] = (int32_t)total;
    total += seq_len[i];
    prev_end = seq_off[i] + seq_len[i];
  }
  // ranks permute the positions 0 .. total-1, so the event segments must be exactly those positions (no [SEP])
  OT_REQUIRE(!rank || (ldr >= total && prev_end == total), "ot_seq_key_valid: ranks need ldr >= the %lld events and "
             "segments without gaps", (long long)total);
  if (B == 0) return OT_OK;
  OT_REQUIRE(valid0 && (nseq == 0 || lens), "ot_seq_key_valid: null operand");
  OT_REQUIRE((int64_t)B * L0 < ((int64_t)1 << 31) * 256, "ot_seq_key_valid: grid too large");
  hipLaunchKernelGGL(seq_key_valid_kernel, dim3(ceil_div((int64_t)B * L0, 256)), dim3(256), 0, (hipStream_t)stream, a,
                     nseq, lens, B, L0, rank, ldr, valid0);
  OT_LAUNCH_CHECK("ot_seq_key_valid");
  return OT_OK;
}
