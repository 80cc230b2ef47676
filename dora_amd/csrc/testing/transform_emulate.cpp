// Host emulation of transform_kernel (transform_device.h), a stand-alone program that
// tests/test_random_arrays_host.py compiles with the host compiler and
// -fsanitize=address,undefined and runs once per case; it is part of no library.
//
// It cuts the transform segments of a compacting plan into launches of kXMaxSegs as launch_pack
// does, fills each launch's XArgs with the product's fill_xargs and runs transform_body for every
// block and every thread of the launch, through a memory policy of plain loads and checked stores:
//   (a) every source is a heap block of its own that ends with the segment's last readable byte
//       (src_len bytes of a bitmap slice, len bytes of offsets), so a read past a bitmap's last
//       byte or past the last offset stops the run under AddressSanitizer; the whole-word loads
//       and stores are the kernel's own casts, whose alignment UBSan checks;
//   (b) the destination is a heap block that ends with the sample's last byte; every store lies
//       inside the sample and inside the region of a transform segment;
//   (c) no output byte is written twice, by any thread of any block of any launch;
//   (d) every byte of every transform segment's region is written.
// The destination, poisoned with 0xA5 where nothing was written, goes to `out_file`.
//
//   transform_emulate spec_file blob_file out_file
//
// `spec_file`: "size dst_mis nseg", then per segment "op aux dst_off len src_len src_mis blob_off":
// the sample's bytes and its address mod 16, and per segment the plan's op, aux, destination
// offset, output bytes and src_len, the source's address mod 16 and where its bytes start in
// `blob_file`.  Exit status 0 and "ok" when every check held.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "transform_device.h"

namespace {

namespace xf = dora::xform;

[[noreturn]] void die(const char* what, int64_t a, int64_t b) {
  std::printf("FAIL %s (%" PRId64 ", %" PRId64 ")\n", what, a, b);
  std::exit(1);
}

struct EmuMem {
  uint8_t* dst;
  uint64_t size;
  std::vector<uint8_t> writes, region;
  uint64_t blk = 0;
  uint64_t words = 0, pieces = 0;  // whole-word and byte-wise offsets stored

  void note(const uint8_t* p, size_t n) {
    if (p < dst || uint64_t(p - dst) + n > size)
      die("store outside the sample", int64_t(p - dst), int64_t(blk));
    for (uint64_t o = uint64_t(p - dst); n--; ++o) {
      if (!region[o]) die("store outside every transform segment", int64_t(o), int64_t(blk));
      if (++writes[o] != 1) die("output byte written twice", int64_t(o), int64_t(blk));
    }
  }
  template <typename T>
  T ld(const uint8_t* p) const {
    return *reinterpret_cast<const T*>(p);
  }
  template <typename T>
  void st(uint8_t* p, T v) {
    note(p, sizeof(T));
    *reinterpret_cast<T*>(p) = v;
    words += sizeof(T) > 1;
  }
  template <typename T>
  T ldu(const uint8_t* p) const {
    T v;
    std::memcpy(&v, p, sizeof(T));
    return v;
  }
  template <typename T>
  void stu(uint8_t* p, T v) {
    note(p, sizeof(T));
    std::memcpy(p, &v, sizeof(T));
    ++pieces;
  }
};

// A heap block of `n` bytes on a 16-byte boundary (one byte when n == 0).
uint8_t* block16(uint64_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, n ? n : 1) != 0) die("out of memory", int64_t(n), 0);
  return static_cast<uint8_t*>(p);
}

std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[1 << 16];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::printf("usage: see the file's head\n");
    return 2;
  }
  FILE* sf = std::fopen(argv[1], "r");
  uint64_t size = 0, dst_mis = 0, nseg = 0;
  if (!sf || std::fscanf(sf, "%" SCNu64 " %" SCNu64 " %" SCNu64, &size, &dst_mis, &nseg) != 3 ||
      dst_mis >= 16 || nseg > (1u << 20)) {
    std::printf("FAIL bad spec\n");
    return 2;
  }
  const std::vector<uint8_t> blob = read_file(argv[2]);
  // the sample: a block that ends with its last byte, at dst_mis mod 16
  uint8_t* dst_block = block16(dst_mis + size);
  EmuMem m;
  m.dst = dst_block + dst_mis;
  m.size = size;
  std::memset(m.dst, 0xA5, size);
  m.writes.assign(size, 0);
  m.region.assign(size, 0);
  std::vector<dora::Segment> segs(nseg);
  std::vector<uint8_t*> blocks(nseg, nullptr);
  for (uint64_t k = 0; k < nseg; ++k) {
    uint64_t op, aux, dst_off, len, src_len, src_mis, blob_off;
    if (std::fscanf(sf, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64
                        " %" SCNu64, &op, &aux, &dst_off, &len, &src_len, &src_mis, &blob_off) != 7 ||
        op < dora::SEG_BITSHIFT || op > dora::SEG_REBASE64 || aux > 7 || src_mis >= 16) {
      std::printf("FAIL bad segment %" PRIu64 "\n", k);
      return 2;
    }
    const uint64_t readable = op == dora::SEG_BITSHIFT ? src_len : len;
    if (blob_off > blob.size() || readable > blob.size() - blob_off || dst_off > size ||
        len > size - dst_off) {
      std::printf("FAIL segment %" PRIu64 " outside the blob or the sample\n", k);
      return 2;
    }
    // the source: a block that ends with its last readable byte, at src_mis mod 16
    blocks[k] = block16(src_mis + readable);
    if (readable) std::memcpy(blocks[k] + src_mis, blob.data() + blob_off, readable);
    segs[k].src = blocks[k] + src_mis;
    segs[k].dst_off = dst_off;
    segs[k].len = len;
    segs[k].op = static_cast<uint32_t>(op);
    segs[k].aux = static_cast<uint32_t>(aux);
    segs[k].src_len = src_len;
    for (uint64_t o = dst_off; o < dst_off + len; ++o)
      if (m.region[o]++) die("transform segments overlap", int64_t(k), int64_t(o));
  }
  std::fclose(sf);

  uint64_t launches = 0, blocks_run = 0, later_blocks = 0, after_long = 0;
  for (size_t j = 0; j < segs.size(); j += xf::kXMaxSegs) {  // launch_pack's loop
    xf::XArgs x;
    std::memset(&x, 0, sizeof(x));
    const size_t n = segs.size() - j < size_t(xf::kXMaxSegs) ? segs.size() - j : xf::kXMaxSegs;
    const uint32_t grid = xf::fill_xargs(x, m.dst, segs.data() + j, n);
    if (!grid) die("too many blocks", int64_t(j), 0);
    for (uint32_t blk = 0; blk < grid; ++blk) {
      m.blk = blk;
      for (uint32_t t = 0; t < uint32_t(xf::kXThreads); ++t) xf::transform_body(x, blk, t, m);
    }
    // which paths ran, for the caller's counts: blocks past the first of their segment, and
    // first blocks of a segment that follows one of two or more blocks
    for (size_t k = 0; k < n; ++k) {
      const uint32_t b0 = k ? x.block_end[k - 1] : 0, nb = x.block_end[k] - b0;
      later_blocks += nb - 1;
      if (k && x.block_end[k - 1] - (k > 1 ? x.block_end[k - 2] : 0) > 1) ++after_long;
    }
    blocks_run += grid;
    ++launches;
  }
  for (uint64_t o = 0; o < size; ++o)
    if (m.region[o] && m.writes[o] != 1) die("byte of a transform segment never written", int64_t(o), 0);
  FILE* f = std::fopen(argv[3], "wb");
  if (!f || (size && std::fwrite(m.dst, 1, size, f) != size)) {
    std::printf("FAIL output file\n");
    return 2;
  }
  std::fclose(f);
  for (uint8_t* b : blocks) std::free(b);
  std::free(dst_block);
  std::printf("ok launches=%" PRIu64 " blocks=%" PRIu64 " later_blocks=%" PRIu64
              " after_long=%" PRIu64 " words=%" PRIu64 " pieces=%" PRIu64 "\n",
              launches, blocks_run, later_blocks, after_long, m.words, m.pieces);
  return 0;
}
