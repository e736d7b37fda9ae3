// bgzf.hip -- a BGZF-compressed FASTA inflated ON THE DEVICE: the members of the file (bgzf_inflate.h: independent gzip members of
// at most 64 KiB of text each, their sizes in header and trailer) are decoded side by side by one launch, so that the compressed
// bytes are what crosses host memory and no host thread runs zlib (ingest.hip: load_fasta_device).
//
// Work mapping: ONE MEMBER PER LANE.  A 3 GB text has ~48 000 members, more than the lanes the kernel keeps resident, so the serial
// decode of a member needs no cooperation inside a wave.  Each lane owns BGZF_TAB_ELEMS 16-bit table entries in LDS (canonical
// count / symbol tables of both sets, the code lengths of a dynamic block): 896 B per lane, 56 KiB per wave of 64 = one block, two
// blocks per CU of 160 KiB.  The entries are interleaved by lane in 32-bit words (entry e of lane l in word (e >> 1) * 64 + l): lanes
// that read the same entry -- the common case at the top of a decode -- hit 64 different banks; lanes deep in different codes
// collide at random like any gather.  The text leaves through a word accumulator: whole aligned words of the member are stored as
// words, the bytes of a word the member shares with its neighbour (first and last) as bytes, so no lane writes a neighbour's byte.
// The CRC-32 of the text is taken as the bytes are put (table in LDS) and compared with the trailer's in the same kernel.
#include "bgzf_dev_io.h"
#include "mxg_internal.h"

namespace mxg {

__global__ __launch_bounds__(BGZF_BLOCK) void k_bgzf_inflate(const unsigned char *__restrict__ comp, uint64_t comp_bytes,
                                                            const BgzfMember *__restrict__ members, uint32_t n_members, unsigned char *text,
                                                            uint64_t text_bytes, uint32_t *__restrict__ status)
{
    __shared__ uint32_t tabs[(BGZF_TAB_ELEMS / 2) * BGZF_BLOCK];
    __shared__ uint32_t crc_tab[256];
    for (uint32_t i = threadIdx.x; i < 256u; i += BGZF_BLOCK) crc_tab[i] = bgzf_crc32_entry(i);
    __syncthreads();
    const uint32_t m = blockIdx.x * BGZF_BLOCK + threadIdx.x;
    if (m >= n_members) return;
    const BgzfMember d = members[m];
    uint32_t st;
    // (the table was made from the file's own numbers: its ranges are checked once more against the two buffers)
    if (d.in_off > comp_bytes || d.in_len > comp_bytes - d.in_off || d.out_off > text_bytes || d.isize > text_bytes - d.out_off) {
        st = BGZF_PLAN;
    } else {
        BgzfDevSrc src{comp + d.in_off, d.in_len};
        BgzfDevSink sink{text + d.out_off, crc_tab};
        BgzfLdsTab tab{reinterpret_cast<uint16_t *>(tabs) + 2u * threadIdx.x};
        st = bgzf_inflate_member(src, sink, tab, d.isize);
        if (sink.pend) sink.flush();
        if (st == BGZF_OK && (sink.crc ^ 0xFFFFFFFFu) != d.crc) st = BGZF_CRC;
    }
    status[1u + m] = st;
    if (st != BGZF_OK) atomicMax(&status[0], st);
}

// status: n_members + 1 words; status[0] = 0 or the largest BgzfStatus any member ended with
int bgzf_inflate_device(mxg_handle *h, const unsigned char *d_comp, uint64_t comp_bytes, const BgzfMember *d_members, uint32_t n_members,
                        unsigned char *d_text, uint64_t text_bytes, uint32_t *d_status, hipStream_t st)
{
    MXG_HIP(h, hipMemsetAsync(d_status, 0, 4, st));
    if (!n_members) return MXG_OK;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((n_members + BGZF_BLOCK - 1) / BGZF_BLOCK), dim3(BGZF_BLOCK), 0, st, d_comp, comp_bytes, d_members,
                       n_members, d_text, text_bytes, d_status);
    MXG_HIP(h, hipGetLastError());
    return MXG_OK;
}

}  // namespace mxg
