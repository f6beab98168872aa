// trunk_plan.hip — the f16x2 ResNet trunk as one native call (rr.h, "native
// ResNet trunk plan").  No kernel lives here: a forward issues the library's
// own entry points (rr_preprocess_u8_ex, rr_amax_f32, rr_stem_pool_h2,
// rr_conv2d_h2, rr_bottleneck_out_h2, rr_maxpool2d) in the order
// networks.ResNet.maps issues them, for the whole batch on the
// caller's stream or for two halves on the plan's two streams, one conv apart.
#include <algorithm>
#include <mutex>
#include <new>

#include "rr_internal.hpp"

struct rr_trunk_plan_s {
  rr_trunk_desc_t d{};
  std::vector<rr_trunk_conv_t> convs;
  int device = 0;
  int n_blocks = 0;
  int out_cout = 0;  // the last stage's output channels
  hipStream_t st[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_gate = nullptr, ev_done[2] = {nullptr, nullptr};
  std::mutex mu;
  long long n_forward = 0, n_two_part = 0, n_side_ops = 0;
};

namespace rr {
namespace {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int conv_out(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }

// One bottleneck of the walk below.
struct Block {
  int k, stage;                      // its number in forward order, its stage
  bool entry, fused;                 // a stage's first block; its conv3 + downsample as one GEMM
  bool stage_end, last;              // a stage's last block; the trunk's
  int stride, s1, s2;                // the block's, conv1's and conv2's, as the stage layout has them
  const rr_trunk_conv_t* down;       // the downsample conv where it is a launch of its own, else NULL
  const rr_trunk_conv_t* c;          // c[0] conv1, c[1] conv2, c[2] conv3 or the fused [W3 | Wd]
  int cin;                           // the block input's channels
  int h, w, h1, w1, ho, wo;          // the maps: block input, after conv1, block output
};

// The one walk over a description's stages and blocks and its conv list (the
// stem first, then per block [downsample,] conv1, conv2, conv3): f(Block) per
// block, the maps following from h x w at the first block's input.  The list
// must hold the layout's count of convs, each with a stride >= 1.
template <class F>
void walk_blocks(const rr_trunk_desc_t& d, const rr_trunk_conv_t* convs, int h, int w, F&& f) {
  const rr_trunk_conv_t* c = convs + 1;
  Block b{};
  b.cin = convs->cout, b.h = h, b.w = w;
  for (b.stage = 0; b.stage < d.n_stages; ++b.stage)
    for (int bi = 0; bi < d.blocks[b.stage]; ++bi, ++b.k) {
      b.entry = bi == 0, b.fused = b.entry && d.fuse_entry[b.stage];
      b.stage_end = bi + 1 == d.blocks[b.stage], b.last = b.stage_end && b.stage + 1 == d.n_stages;
      b.stride = (b.entry && b.stage > 0) ? 2 : 1;
      b.s1 = d.stride_on ? b.stride : 1, b.s2 = d.stride_on ? 1 : b.stride;
      b.down = (b.entry && !b.fused) ? c++ : nullptr;
      b.c = c;
      b.h1 = conv_out(b.h, c[0].kh, c[0].stride, c[0].pad), b.w1 = conv_out(b.w, c[0].kw, c[0].stride, c[0].pad);
      b.ho = conv_out(b.h1, c[1].kh, c[1].stride, c[1].pad), b.wo = conv_out(b.w1, c[1].kw, c[1].stride, c[1].pad);
      f(b);
      b.cin = c[2].cout, b.h = b.ho, b.w = b.wo;
      c += 3;
    }
}

// One launch of a part's sequence.
struct Op {
  enum Kind { ZERO, PREPROCESS, AMAX, STEM_POOL, CONV, MAXPOOL, ENTRY } kind;
  int hook = -1;  // the conv's number as part 1's lag counts it, -1: not counted
  const rr_trunk_conv_t* c = nullptr;
  const void* x = nullptr;       // input (uint8 pixels for PREPROCESS)
  const unsigned* xa = nullptr;  // its record
  const float* x2 = nullptr;     // residual (CONV) or the block input (ENTRY)
  const unsigned* x2a = nullptr;
  void* y = nullptr;
  unsigned* ya = nullptr;
  int b = 0, h = 0, w = 0;       // input geometry
  int h2 = 0, w2 = 0;            // ENTRY: the block input's
  long long n = 0;               // AMAX: floats; ZERO: bytes
};

// Buffer sizes (floats per image) and records of a trunk at H x W.
struct Shape {
  size_t max_x = 0, max_y = 0, max_idn = 0;
  int n_rec = 0;
  int oh = 0, ow = 0;      // x4's map
  int h3 = 0, w3 = 0, c3 = 0;  // x3's
};

Shape trunk_shape(const rr_trunk_plan_s* p, int hgt, int wid) {
  Shape s;
  const rr_trunk_conv_t* c = p->convs.data();
  s.n_rec = 2 + 3 * p->n_blocks;
  s.max_x = (size_t)hgt * wid * 4;
  int h = conv_out(hgt, c->kh, c->stride, c->pad), w = conv_out(wid, c->kw, c->stride, c->pad);
  if (!p->d.fuse_stem_pool) s.max_y = (size_t)h * w * c->cout;
  h = (h - 1) / 2 + 1;
  w = (w - 1) / 2 + 1;
  s.max_x = std::max(s.max_x, (size_t)h * w * c->cout);
  walk_blocks(p->d, c, h, w, [&](const Block& b) {
    // (a validated downsample conv has the block's stride: its map is the block's output map)
    if (b.down) s.max_idn = std::max(s.max_idn, (size_t)b.ho * b.wo * b.down->cout);
    s.max_y = std::max(s.max_y, std::max((size_t)b.h1 * b.w1 * b.c[0].cout, (size_t)b.ho * b.wo * b.c[1].cout));
    s.max_x = std::max(s.max_x, (size_t)b.ho * b.wo * b.c[2].cout);
    if (b.stage == 2 && b.stage_end) s.h3 = b.ho, s.w3 = b.wo, s.c3 = b.c[2].cout;
    s.oh = b.ho, s.ow = b.wo;
  });
  return s;
}

// Bytes of one part's workspace at b images: two block buffers, two
// inner buffers, the projected identity where a stage entry is not fused,
// and the records.
struct PartWs {
  size_t x[2], y[2], idn, rec, total;
};

PartWs part_layout(const Shape& s, int b) {
  PartWs L{};
  size_t o = 0;
  for (int i = 0; i < 2; ++i) L.x[i] = o, o = up256(o + s.max_x * b * 4);
  for (int i = 0; i < 2; ++i) L.y[i] = o, o = up256(o + s.max_y * b * 4);
  L.idn = o, o = up256(o + s.max_idn * b * 4);
  L.rec = o, o = up256(o + (size_t)s.n_rec * RR_AMAX_SLOTS * 4);
  L.total = o;
  return L;
}

bool shape_ok(const rr_trunk_plan_s* p, int b, int hgt, int wid) {
  return p && b >= 0 && hgt > 0 && wid > 0;
}

// rr.h's rule: two parts only while each still gives the last stage's output
// at least two 256 x 256 tiles per compute unit.
int pick_parts(rr_handle_s* h, const rr_trunk_plan_s* p, int b, int hgt, int wid) {
  if (b < 2 || h->tune.trunk_parts == 1) return 1;
  if (h->tune.trunk_parts == 2) return 2;
  const Shape s = trunk_shape(p, hgt, wid);
  const long long rows = (long long)(b / 2) * s.oh * s.ow;
  const long long tiles = ((rows + 255) / 256) * (p->out_cout / 256);
  return tiles >= 2LL * device_cu_count(h) ? 2 : 1;
}

// The launches of one part: images [0, b) at img, outputs at x4 / x3 (this
// part's rows), records rec_x4 (shared) and rec_x3 (NULL: the part's own).
void build_ops(const rr_trunk_plan_s* p, const Shape& s, const uint8_t* img, int b, int hgt, int wid, char* ws,
               float* x4, unsigned* rec_x4, float* x3, unsigned* rec_x3, std::vector<Op>& ops,
               unsigned** own_x3_rec) {
  const PartWs L = part_layout(s, b);
  float* X[2] = {(float*)(ws + L.x[0]), (float*)(ws + L.x[1])};
  float* Y[2] = {(float*)(ws + L.y[0]), (float*)(ws + L.y[1])};
  float* IDN = (float*)(ws + L.idn);
  unsigned* rec = (unsigned*)(ws + L.rec);
  auto R = [&](int i) { return rec + (size_t)i * RR_AMAX_SLOTS; };
  const rr_trunk_conv_t* c = p->convs.data();
  Op o;
  o = Op{};
  o.kind = Op::ZERO, o.y = rec, o.n = (long long)s.n_rec * RR_AMAX_SLOTS * 4;
  ops.push_back(o);
  o = Op{};
  o.kind = Op::PREPROCESS, o.x = img, o.y = X[1], o.b = b, o.h = hgt, o.w = wid;
  ops.push_back(o);
  o = Op{};
  o.kind = Op::AMAX, o.x = X[1], o.ya = R(0), o.n = (long long)b * hgt * wid * 4;
  ops.push_back(o);
  int h = conv_out(hgt, c->kh, c->stride, c->pad), w = conv_out(wid, c->kw, c->stride, c->pad);
  o = Op{};
  o.c = c, o.x = X[1], o.xa = R(0), o.ya = R(1), o.b = b, o.h = hgt, o.w = wid, o.hook = 0;
  if (p->d.fuse_stem_pool) {
    o.kind = Op::STEM_POOL, o.y = X[0];
    ops.push_back(o);
  } else {
    o.kind = Op::CONV, o.y = Y[0], o.hook = -1;
    ops.push_back(o);
    o = Op{};
    o.kind = Op::MAXPOOL, o.c = c, o.x = Y[0], o.y = X[0], o.b = b, o.h = h, o.w = w, o.hook = 0;
    ops.push_back(o);
  }
  h = (h - 1) / 2 + 1;
  w = (w - 1) / 2 + 1;
  const float* cur = X[0];
  int cur_i = 0;  // which workspace block buffer holds cur (-1: an output tensor)
  const unsigned* xa = R(1);
  walk_blocks(p->d, c, h, w, [&](const Block& k) {
    const int r = 2 + 3 * k.k, ci = 1 + 3 * k.k;
    const float* idn = cur;
    if (k.down) {
      o = Op{};
      o.kind = Op::CONV, o.c = k.down, o.x = cur, o.xa = xa, o.y = IDN, o.b = b, o.h = k.h, o.w = k.w;
      ops.push_back(o);
      idn = IDN;
    }
    o = Op{};
    o.kind = Op::CONV, o.c = k.c, o.x = cur, o.xa = xa, o.y = Y[0], o.ya = R(r), o.b = b, o.h = k.h, o.w = k.w, o.hook = ci;
    ops.push_back(o);
    o = Op{};
    o.kind = Op::CONV, o.c = k.c + 1, o.x = Y[0], o.xa = R(r), o.y = Y[1], o.ya = R(r + 1), o.b = b, o.h = k.h1, o.w = k.w1,
    o.hook = ci + 1;
    ops.push_back(o);
    // where the block's output goes: an output tensor, or the free block buffer
    float* dst;
    unsigned* dsta = R(r + 2);
    int dst_i = -1;
    if (k.last) {
      dst = x4, dsta = rec_x4;
    } else if (k.stage_end && k.stage == 2 && x3) {
      dst = x3;
      if (rec_x3) dsta = rec_x3;
      else *own_x3_rec = dsta;
    } else {
      dst_i = cur_i == 0 ? 1 : 0;
      dst = X[dst_i];
    }
    o = Op{};
    o.c = k.c + 2, o.x = Y[1], o.xa = R(r + 1), o.y = dst, o.ya = dsta, o.b = b, o.h = k.ho, o.w = k.wo, o.hook = ci + 2;
    if (k.fused) {
      o.kind = Op::ENTRY, o.x2 = cur, o.x2a = xa, o.h2 = k.h, o.w2 = k.w;
    } else {
      o.kind = Op::CONV, o.x2 = idn;
    }
    ops.push_back(o);
    cur = dst, cur_i = dst_i, xa = dsta;
  });
}

int issue(rr_handle_s* h, const rr_trunk_plan_s* p, const Op& o, hipStream_t s) {
  const rr_trunk_conv_t* c = o.c;
  switch (o.kind) {
    case Op::ZERO:
      return check_hip(h, hipMemsetAsync(o.y, 0, (size_t)o.n, s), "rr_trunk_h2: memset");
    case Op::PREPROCESS:
      return rr_preprocess_u8_ex(h, (const uint8_t*)o.x, o.b, o.h, o.w, p->d.mean, p->d.std, 4, (float*)o.y, s);
    case Op::AMAX:
      return rr_amax_f32(h, (const float*)o.x, o.n, o.ya, s);
    case Op::STEM_POOL:
      return rr_stem_pool_h2(h, (const float*)o.x, o.xa, o.b, o.h, o.w, c->w2, c->w_iscale, c->bias, c->cout, c->kh,
                             c->kw, c->stride, c->pad, (float*)o.y, o.ya, s);
    case Op::MAXPOOL:
      return rr_maxpool2d(h, (const float*)o.x, o.b, o.h, o.w, c->cout, 3, 2, 1, (float*)o.y, s);
    case Op::CONV:
      return rr_conv2d_h2(h, (const float*)o.x, o.xa, o.b, o.h, o.w, c->cin, c->w2, c->w_iscale, c->bias, c->cout,
                          c->kh, c->kw, c->stride, c->pad, o.x2, c->relu, (float*)o.y, o.ya, s);
    case Op::ENTRY: {
      const int planes = (c - 1)->cout;  // conv3's rows are [W3 | Wd]: conv2's planes + the block's input channels
      return rr_bottleneck_out_h2(h, (const float*)o.x, o.xa, o.b, o.h, o.w, planes, o.x2, o.x2a, o.h2, o.w2,
                                  c->cin - planes, c->stride, c->w2, c->w_iscale, c->bias, c->cout, (float*)o.y, o.ya,
                                  s);
    }
  }
  return RR_EINVAL;
}

}  // namespace
}  // namespace rr

using namespace rr;

extern "C" {

int rr_trunk_h2_create(rr_handle_t h, const rr_trunk_desc_t* d, rr_trunk_plan_t* out) {
  RR_ENTRY(h);
  if (!out) return set_error(h, RR_EINVAL, "rr_trunk_h2_create: null out");
  *out = nullptr;
  if (!d || !d->convs || d->n_stages < 1 || d->n_stages > RR_TRUNK_MAX_STAGES || d->lag < 0 ||
      (d->stride_on != 0 && d->stride_on != 1))
    return set_error(h, RR_EINVAL, "rr_trunk_h2_create: bad description");
  // the conv list against the stage layout: count, channel chain, strides
  int need = 1, n_blocks = 0;
  for (int li = 0; li < d->n_stages; ++li) {
    if (d->blocks[li] < 1) return set_error(h, RR_EINVAL, "rr_trunk_h2_create: a stage without blocks");
    need += 3 * d->blocks[li] + (d->fuse_entry[li] ? 0 : 1);
    n_blocks += d->blocks[li];
  }
  if (need != d->n_convs) return set_error(h, RR_EINVAL, "rr_trunk_h2_create: n_convs does not fit the stage layout");
  for (int i = 0; i < d->n_convs; ++i) {
    const rr_trunk_conv_t& c = d->convs[i];
    if (!c.w2 || !c.w_iscale || c.cin <= 0 || c.cout <= 0 || c.kh <= 0 || c.kw <= 0 || c.stride <= 0 || c.pad < 0)
      return set_error(h, RR_EINVAL, "rr_trunk_h2_create: bad conv entry");
  }
  const rr_trunk_conv_t* c = d->convs;
  if (c->cin != 4 || (d->fuse_stem_pool && c->cout != 64) || !c->relu)
    return set_error(h, RR_EINVAL, "rr_trunk_h2_create: the stem reads NHWC4, has a ReLU and, fused with its pool, cout 64");
  int ch = c->cout;
  bool ok = true;
  walk_blocks(*d, c, 0, 0, [&](const Block& b) {
    const rr_trunk_conv_t* c = b.c;
    if (b.down)
      ok = ok && b.down->cin == b.cin && b.down->kh == 1 && b.down->kw == 1 && b.down->stride == b.stride &&
           b.down->pad == 0 && !b.down->relu && !b.down->residual && b.down->cout == c[2].cout;
    ok = ok && c[0].cin == b.cin && c[0].kh == 1 && c[0].kw == 1 && c[0].stride == b.s1 && c[0].pad == 0 && c[0].relu;
    ok = ok && c[1].cin == c[0].cout && c[1].kh == 3 && c[1].kw == 3 && c[1].stride == b.s2 && c[1].pad == 1 && c[1].relu;
    ok = ok && c[2].kh == 1 && c[2].kw == 1 && c[2].pad == 0 && c[2].relu;
    if (b.fused)
      ok = ok && c[2].cin == c[1].cout + b.cin && c[2].stride == b.stride && !c[2].residual && c[2].cout % 256 == 0;
    else
      ok = ok && c[2].cin == c[1].cout && c[2].stride == 1 && c[2].residual && (b.entry || c[2].cout == b.cin);
    ch = c[2].cout;
  });
  if (!ok) return set_error(h, RR_EINVAL, "rr_trunk_h2_create: a block's convs do not fit the layout");
  rr_trunk_plan_s* p = new (std::nothrow) rr_trunk_plan_s();
  if (!p) return set_error(h, RR_EINVAL, "rr_trunk_h2_create: out of memory");
  p->d = *d;
  p->convs.assign(d->convs, d->convs + d->n_convs);
  p->d.convs = p->convs.data();
  p->device = h->device;
  p->n_blocks = n_blocks;
  p->out_cout = ch;
  hipError_t e = hipSuccess;
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&p->st[i], hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev_gate, hipEventDisableTiming);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&p->ev_done[i], hipEventDisableTiming);
  if (e != hipSuccess) {
    (void)rr_trunk_h2_destroy(h, p);
    return check_hip(h, e, "rr_trunk_h2_create: streams and events");
  }
  *out = p;
  return RR_OK;
}

int rr_trunk_h2_destroy(rr_handle_t h, rr_trunk_plan_t p) {
  RR_ENTRY(h);
  if (!p) return RR_OK;
  for (int i = 0; i < 2; ++i) {
    if (p->st[i]) {
      (void)hipStreamSynchronize(p->st[i]);
      (void)hipStreamDestroy(p->st[i]);
    }
    if (p->ev_done[i]) (void)hipEventDestroy(p->ev_done[i]);
  }
  if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
  if (p->ev_gate) (void)hipEventDestroy(p->ev_gate);
  delete p;
  return RR_OK;
}

size_t rr_trunk_h2_workspace_size(rr_trunk_plan_t p, int b, int hgt, int wid, int parts) {
  if (!shape_ok(p, b, hgt, wid) || (parts != 1 && parts != 2)) return 0;
  const Shape s = trunk_shape(p, hgt, wid);
  if (parts == 1 || b < 2) return part_layout(s, b).total;
  return part_layout(s, b / 2).total + part_layout(s, b - b / 2).total;
}

int rr_trunk_h2_parts(rr_handle_t h, rr_trunk_plan_t p, int b, int hgt, int wid) {
  RR_ENTRY(h);
  if (!shape_ok(p, b, hgt, wid)) return set_error(h, RR_EINVAL, "rr_trunk_h2_parts: null plan, b < 0, H < 1 or W < 1");
  return pick_parts(h, p, b, hgt, wid);
}

int rr_trunk_h2_counters(rr_trunk_plan_t p, long long* out3) {
  if (!p || !out3) return RR_EINVAL;
  std::lock_guard<std::mutex> lk(p->mu);
  out3[0] = p->n_forward, out3[1] = p->n_two_part, out3[2] = p->n_side_ops;
  return RR_OK;
}

int rr_trunk_h2_forward_u8(rr_handle_t h, rr_trunk_plan_t p, const uint8_t* img, int b, int hgt, int wid,
                           float* out_x4, unsigned* out_x4_amax, float* out_x3, unsigned* out_x3_amax,
                           void* workspace, size_t workspace_bytes, void* stream) {
  RR_ENTRY(h);
  if (!p) return set_error(h, RR_EINVAL, "rr_trunk_h2_forward_u8: null plan");
  if (p->device != h->device) return set_error(h, RR_EINVAL, "rr_trunk_h2_forward_u8: the plan belongs to another device's handle");
  if (!shape_ok(p, b, hgt, wid))
    return set_error(h, RR_EINVAL, "rr_trunk_h2_forward_u8: need b >= 0, H >= 1 and W >= 1");
  if (b == 0) return RR_OK;
  if (!img || !out_x4 || !out_x4_amax || (out_x3 == nullptr) != (out_x3_amax == nullptr) ||
      (out_x3 && p->d.n_stages < 4) || ((uintptr_t)out_x4 & 15) || ((uintptr_t)out_x3 & 15))
    return set_error(h, RR_EINVAL, "rr_trunk_h2_forward_u8: null or misaligned pointer (out_x3 with its record, >= 4 stages)");
  std::lock_guard<std::mutex> lk(p->mu);
  const int parts = pick_parts(h, p, b, hgt, wid);
  const Shape s = trunk_shape(p, hgt, wid);
  if (s.oh <= 0 || s.ow <= 0) return set_error(h, RR_EINVAL, "rr_trunk_h2_forward_u8: empty output");
  const int nb[2] = {parts == 2 ? b / 2 : b, parts == 2 ? b - b / 2 : 0};
  const size_t need = part_layout(s, nb[0]).total + (parts == 2 ? part_layout(s, nb[1]).total : 0);
  if (!workspace || ((uintptr_t)workspace & 255) || workspace_bytes < need)
    return set_error(h, RR_EWORKSPACE, "rr_trunk_h2_forward_u8: workspace too small (rr_trunk_h2_workspace_size) or not 256-B aligned");
  hipStream_t cs = (hipStream_t)stream;
  ++p->n_forward;
  if (int rc = check_hip(h, hipMemsetAsync(out_x4_amax, 0, RR_AMAX_SLOTS * 4, cs), "rr_trunk_h2: memset")) return rc;
  if (out_x3_amax)
    if (int rc = check_hip(h, hipMemsetAsync(out_x3_amax, 0, RR_AMAX_SLOTS * 4, cs), "rr_trunk_h2: memset")) return rc;
  std::vector<Op> ops[2];
  unsigned* own_x3[2] = {nullptr, nullptr};
  if (parts == 1) {
    build_ops(p, s, img, b, hgt, wid, (char*)workspace, out_x4, out_x4_amax, out_x3, out_x3_amax, ops[0], &own_x3[0]);
    for (const Op& o : ops[0])
      if (int rc = issue(h, p, o, cs)) return rc;
    return RR_OK;
  }
  // two parts: part 1's rows follow part 0's in the images and in both outputs
  const size_t x4_img = (size_t)s.oh * s.ow * p->out_cout, x3_img = (size_t)s.h3 * s.w3 * s.c3;
  char* ws1 = (char*)workspace + part_layout(s, nb[0]).total;
  build_ops(p, s, img, nb[0], hgt, wid, (char*)workspace, out_x4, out_x4_amax, out_x3, nullptr, ops[0], &own_x3[0]);
  build_ops(p, s, img + (size_t)nb[0] * hgt * wid * 3, nb[1], hgt, wid, ws1, out_x4 + nb[0] * x4_img, out_x4_amax,
            out_x3 ? out_x3 + nb[0] * x3_img : nullptr, nullptr, ops[1], &own_x3[1]);
  ++p->n_two_part;
  // fork
  if (int rc = check_hip(h, hipEventRecord(p->ev_fork, cs), "rr_trunk_h2: fork")) return rc;
  int rc = RR_OK;
  for (int i = 0; i < 2 && !rc; ++i) {
    rc = check_hip(h, hipStreamWaitEvent(p->st[i], p->ev_fork, 0), "rr_trunk_h2: fork wait");
    ++p->n_side_ops;
  }
  // part 0's launch k, then part 1's launch k - (the gate's place): neither
  // queue runs dry while the other is filled; part 1 starts once part 0 has
  // recorded the gate after its lag-th conv (no gate when lag is past the end)
  int last_hook = 0;
  for (const Op& o : ops[0]) last_hook = std::max(last_hook, o.hook);
  const bool gated = p->d.lag <= last_hook;
  bool open = !gated;
  size_t ia = 0, ib = 0;
  while (!rc && (ia < ops[0].size() || ib < ops[1].size())) {
    if (ia < ops[0].size()) {
      const Op& o = ops[0][ia++];
      rc = issue(h, p, o, p->st[0]);
      ++p->n_side_ops;
      if (!rc && gated && o.hook == p->d.lag) {
        rc = check_hip(h, hipEventRecord(p->ev_gate, p->st[0]), "rr_trunk_h2: gate");
        if (!rc) rc = check_hip(h, hipStreamWaitEvent(p->st[1], p->ev_gate, 0), "rr_trunk_h2: gate wait");
        p->n_side_ops += 2;
        open = true;
      }
    }
    if (!rc && open && ib < ops[1].size()) {
      rc = issue(h, p, ops[1][ib++], p->st[1]);
      ++p->n_side_ops;
    }
  }
  // join, also after a failed launch: the caller's stream must not run ahead
  // of what the plan's streams were given
  for (int i = 0; i < 2; ++i) {
    int r2 = check_hip(h, hipEventRecord(p->ev_done[i], p->st[i]), "rr_trunk_h2: join");
    if (!r2) r2 = check_hip(h, hipStreamWaitEvent(cs, p->ev_done[i], 0), "rr_trunk_h2: join wait");
    p->n_side_ops += 1;
    if (!rc) rc = r2;
  }
  // x3's record: each part kept its own (its next conv's split scale); fold both
  if (!rc && out_x3_amax)
    for (int i = 0; i < 2 && !rc; ++i)
      rc = rr_amax_f32(h, reinterpret_cast<const float*>(own_x3[i]), RR_AMAX_SLOTS, out_x3_amax, cs);
  return rc;
}

}  // extern "C"
