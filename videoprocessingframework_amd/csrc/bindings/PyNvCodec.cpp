// PyNvCodec.cpp — pybind11 module `_PyNvCodec`: the Python API of the surface path, name for name with
// the reference's bindings (src/PyNvCodec/src/PyNvCodec.cpp:208-461 module + enums, PySurface.cpp:163-492,
// PySurfaceConverter.cpp:80-120, PySurfaceResizer.cpp:66-102, PySurfaceRemaper.cpp:70-107,
// PyFrameUploader.cpp:104-161, PySurfaceDownloader.cpp:119-189, PyBufferUploader.cpp:48-96,
// PyCudaBufferDownloader.cpp:50-104) over the HIP Task layer in ../tc.
//
// `context` arguments are opaque device cookies on ROCm (0 = current device, see MemoryInterfaces.hpp);
// `stream` arguments are hipStream_t values (torch.cuda.Stream().cuda_stream works).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "Tasks.hpp"
#include "vpf_hip.h"
#ifdef VPF_WITH_LIBAV
#include <map>

#include "FfmpegFeeder.hpp"
#endif

namespace py = pybind11;
using namespace VPF;

namespace {
constexpr auto TASK_EXEC_SUCCESS = TaskExecStatus::TASK_EXEC_SUCCESS;
constexpr auto TASK_EXEC_FAIL = TaskExecStatus::TASK_EXEC_FAIL;

HipContext ctx_of(int gpu) { return HipResMgr::Instance().GetCtx((size_t)gpu); }
HipStream str_of(int gpu) { return HipResMgr::Instance().GetStream((size_t)gpu); }

std::string plane_repr(SurfacePlane* p, int indent = 0) {
  if (!p) return {};
  const std::string sp(indent, ' ');
  std::stringstream ss;
  ss << sp << "Owns mem:  " << p->OwnMemory() << "\n" << sp << "Width:     " << p->Width() << "\n"
     << sp << "Height:    " << p->Height() << "\n" << sp << "Pitch:     " << p->Pitch() << "\n"
     << sp << "Elem size: " << p->ElemSize() << "\n" << sp << "HIP ctx:   " << p->GetContext() << "\n"
     << sp << "HIP ptr:   " << p->GpuMem() << "\n";
  return ss.str();
}
std::string surface_repr(Surface* s) {
  if (!s) return {};
  std::stringstream ss;
  if (s->Empty()) {
    ss << "Empty surface\nFormat:           " << PixelFormatName(s->PixelFormat()) << "\n";
    return ss.str();
  }
  ss << "Width:            " << s->Width() << "\nHeight:           " << s->Height()
     << "\nFormat:           " << PixelFormatName(s->PixelFormat()) << "\nPitch:            " << s->Pitch()
     << "\nElem size(bytes): " << s->ElemSize() << "\n";
  for (uint32_t i = 0; i < s->NumPlanes() && s->GetSurfacePlane(i); i++) ss << "Plane " << i << "\n" << plane_repr(s->GetSurfacePlane(i), 2) << "\n";
  return ss.str();
}

// deep copy src -> dst, plane by plane, then wait (PySurface.cpp:54-81)
void copy_surface(Surface& src, Surface& dst, HipContext ctx, HipStream str) {
  if (src.Empty() || dst.Empty()) return;
  src.Export(dst, ctx, str, 0, 0, src.Width(), src.Height(), 0, 0);
}
void check_same(Surface& a, Surface& b) {
  if (a.PixelFormat() != b.PixelFormat()) throw std::runtime_error("Surfaces have different pixel formats");
  if (a.Width() != b.Width() || a.Height() != b.Height()) throw std::runtime_error("Surfaces have different size");
}
std::shared_ptr<Surface> make_surface(Pixel_Format f, uint32_t w, uint32_t h, HipContext ctx) {
  Surface* s = Surface::Make(f, w, h, ctx);
  if (!s) throw std::invalid_argument("Surface.Make: unsupported pixel format");
  return std::shared_ptr<Surface>(s);
}
std::shared_ptr<Surface> empty_surface(Pixel_Format f) { return std::shared_ptr<Surface>(Surface::Make(f)); }

// The planes of `n` tensor frames of w x h at device address `base`, as the Task layer's tensor entries take them.  Planar: three per frame,
// element (i, c, y, x) at base + i frame_stride + c plane_stride + y row_pitch + x elem (strides in bytes, 0 = contiguous NCHW).  channels_last:
// ONE per frame, element (i, c, y, x) at base + i frame_stride + y row_pitch + (3 x + c) elem (plane_stride ignored, 0 = contiguous NHWC), and
// VPF_TENSOR_NHWC is set in `norm`.
bool tensor_planes(uint64_t base, uint32_t dtype, size_t n, uint64_t w, uint64_t h, uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride,
                   bool channels_last, vpf_tensor_norm& norm, std::vector<vpf_plane>& planes) {
  const uint64_t elem = dtype == VPF_TENSOR_F32 ? 4 : 2;
  if (!row_pitch) row_pitch = (channels_last ? 3 : 1) * w * elem;
  if (channels_last) plane_stride = 0;
  else if (!plane_stride) plane_stride = h * row_pitch;
  if (!frame_stride) frame_stride = channels_last ? h * row_pitch : 3 * plane_stride;
  if (row_pitch > 0xffffffffull) return false;
  const size_t per = channels_last ? 1 : 3;
  if (channels_last) norm.flags |= VPF_TENSOR_NHWC;
  planes.resize(per * n);
  for (size_t i = 0; i < n; i++)
    for (size_t c = 0; c < per; c++) {
      planes[per * i + c].ptr = (void*)(uintptr_t)(base + i * frame_stride + c * plane_stride);
      planes[per * i + c].pitch = (uint32_t)row_pitch;
      planes[per * i + c].reserved = 0;
    }
  return true;
}

// host-memory "device" allocator: lets CPU-only unit tests build Surfaces (geometry, dispatch, error paths)
void* host_alloc(size_t n, int, void*) { return std::calloc(n ? n : 1, 1); }
void host_free(void* p, int, void*) { std::free(p); }

// ------------------------------------------------------------------------------------------------
class PySurfaceConverter {
  std::unique_ptr<ConvertSurface> conv_;
  std::unique_ptr<Buffer> ctx_buf_;
  Pixel_Format out_fmt_;

public:
  PySurfaceConverter(uint32_t w, uint32_t h, Pixel_Format in, Pixel_Format out, HipContext ctx, HipStream str) : out_fmt_(out) {
    conv_.reset(ConvertSurface::Make(w, h, in, out, ctx, str));
    ctx_buf_.reset(Buffer::MakeOwnMem(sizeof(ColorspaceConversionContext)));
  }
  Pixel_Format GetFormat() const { return out_fmt_; }
  void SetOutputReuseHint(bool on) { conv_->SetOutputReused(on); }
  bool GetOutputReuseHint() const { return conv_->GetOutputReused(); }
  // PySurfaceConverter.cpp:50-74: returns a NON-OWNING alias of the task's single output surface (overwritten by
  // the next Execute); failure of any kind = an Empty() surface
  std::shared_ptr<Surface> Execute(std::shared_ptr<Surface> src, std::shared_ptr<ColorspaceConversionContext> cc) {
    if (!src) return empty_surface(out_fmt_);
    conv_->ClearInputs();
    conv_->SetInput(src.get(), 0U);
    if (cc) {
      ctx_buf_->CopyFrom(sizeof(ColorspaceConversionContext), cc.get());
      conv_->SetInput(ctx_buf_.get(), 1U);
    }
    if (TASK_EXEC_SUCCESS != conv_->Execute()) return empty_surface(out_fmt_);
    auto* out = static_cast<Surface*>(conv_->GetOutput(0U));
    return std::shared_ptr<Surface>(out ? out->Clone() : Surface::Make(out_fmt_));
  }
  // additive: n surfaces in, n caller-owned surfaces out, one dispatch per 32 frames
  bool ExecuteBatch(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<std::shared_ptr<Surface>>& dst,
                    std::shared_ptr<ColorspaceConversionContext> cc) {
    if (src.size() != dst.size() || src.empty()) return false;
    std::vector<Surface*> a, b;
    for (auto& s : src) a.push_back(s.get());
    for (auto& d : dst) b.push_back(d.get());
    return TASK_EXEC_SUCCESS == conv_->RunBatch(a.data(), b.data(), (uint32_t)a.size(), cc.get());
  }
};

// additive: fused conversion + bilinear resize (ConvertResizeSurface), same calling conventions as PySurfaceConverter
class PySurfaceConvertResizer {
  std::unique_ptr<ConvertResizeSurface> task_;
  std::unique_ptr<Buffer> ctx_buf_;
  Pixel_Format out_fmt_;

public:
  PySurfaceConvertResizer(uint32_t sw, uint32_t sh, Pixel_Format in, uint32_t dw, uint32_t dh, Pixel_Format out, HipContext ctx, HipStream str)
      : out_fmt_(out), task_dst_w_(dw), task_dst_h_(dh) {
    task_.reset(ConvertResizeSurface::Make(sw, sh, in, dw, dh, out, ctx, str));
    ctx_buf_.reset(Buffer::MakeOwnMem(sizeof(ColorspaceConversionContext)));
  }
  Pixel_Format GetFormat() const { return out_fmt_; }
  std::shared_ptr<Surface> Execute(std::shared_ptr<Surface> src, std::shared_ptr<ColorspaceConversionContext> cc) {
    if (!src) return empty_surface(out_fmt_);
    task_->ClearInputs();
    task_->SetInput(src.get(), 0U);
    if (cc) {
      ctx_buf_->CopyFrom(sizeof(ColorspaceConversionContext), cc.get());
      task_->SetInput(ctx_buf_.get(), 1U);
    }
    if (TASK_EXEC_SUCCESS != task_->Execute()) return empty_surface(out_fmt_);
    auto* out = static_cast<Surface*>(task_->GetOutput(0U));
    return std::shared_ptr<Surface>(out ? out->Clone() : Surface::Make(out_fmt_));
  }
  bool ExecuteBatch(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<std::shared_ptr<Surface>>& dst,
                    std::shared_ptr<ColorspaceConversionContext> cc) {
    if (src.size() != dst.size() || src.empty()) return false;
    std::vector<Surface*> a, b;
    for (auto& s : src) a.push_back(s.get());
    for (auto& d : dst) b.push_back(d.get());
    return TASK_EXEC_SUCCESS == task_->RunBatch(a.data(), b.data(), (uint32_t)a.size(), cc.get());
  }
  // channels_last (every *ToTensor entry): the tensor is [n, dh, dw, 3] in memory (torch.channels_last of a logical [n, 3, dh, dw]): element
  // (i, c, y, x) at dst + i frame_stride + y row_pitch + (3 x + c) elem; plane_stride is ignored, row_pitch 0 = 3 dw elem, frame_stride 0 = dh row_pitch;
  // ONE plane per frame / job goes to the Task layer (VPF_TENSOR_NHWC)
  // additive: n surfaces -> a normalised planar tensor [n, 3, dh, dw] of f32 / f16 / bf16 at device address `dst` (vpf_convert_resize_tensor):
  // element (i, c, y, x) at dst + i frame_stride + c plane_stride + y row_pitch + x elem (bytes; 0 = contiguous NCHW).  mean / std are
  // torchvision's (values of [0, 1] pixels), per output channel; scale = 1 / (255 std) and bias = -mean / std are computed in double.
  static vpf_tensor_norm norm_of(uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std, bool bgr) {
    if (mean.size() != 3 || std.size() != 3) throw std::invalid_argument("mean and std need three values each");
    vpf_tensor_norm norm;
    std::memset(&norm, 0, sizeof(norm));
    for (int c = 0; c < 3; c++) {
      if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || !(std[c] > 0.0)) throw std::invalid_argument("mean must be finite and std finite and > 0");
      norm.scale[c] = (float)(1.0 / (255.0 * std[c]));
      norm.bias[c] = (float)(-mean[c] / std[c]);
      if (!std::isfinite(norm.scale[c]) || !std::isfinite(norm.bias[c])) throw std::invalid_argument("mean / std give a scale or bias beyond fp32");
    }
    norm.dtype = dtype;
    norm.flags = bgr ? VPF_TENSOR_BGR : 0u;
    return norm;
  }
  bool ExecuteToTensor(const std::vector<std::shared_ptr<Surface>>& src, uint64_t dst, uint32_t dtype, const std::vector<double>& mean,
                       const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc, bool bgr, uint64_t row_pitch,
                       uint64_t plane_stride, uint64_t frame_stride, bool channels_last) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (src.empty() || !dst) return false;
    std::vector<Surface*> a;
    std::vector<vpf_plane> planes;
    if (!tensor_planes(dst, dtype, src.size(), task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    for (size_t i = 0; i < src.size(); i++) a.push_back(src[i].get());
    return TASK_EXEC_SUCCESS == task_->RunTensor(a.data(), (uint32_t)a.size(), planes.data(), norm, cc.get());
  }
  // additive: K rectangles of surfaces -> a normalised planar tensor [K, 3, dh, dw] at device address `dst` (vpf_convert_resize_tensor_rois):
  // rois[i] = (surface index, x, y, w, h) in luma pixels, any integer offset, inside the surface; tensor layout and mean / std as ExecuteToTensor
  bool ExecuteRoisToTensor(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<std::array<int64_t, 5>>& rois, uint64_t dst, uint32_t dtype,
                           const std::vector<double>& mean, const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc, bool bgr,
                           uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride, bool channels_last) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (src.empty() || rois.empty() || !dst) return false;
    std::vector<vpf_plane> planes;
    if (!tensor_planes(dst, dtype, rois.size(), task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    std::vector<uint32_t> index(rois.size());
    std::vector<vpf_rect> rects(rois.size());
    for (size_t i = 0; i < rois.size(); i++) {
      for (int k = 0; k < 5; k++)
        if (rois[i][k] < 0 || rois[i][k] > 0xffffffffll) return false;
      index[i] = (uint32_t)rois[i][0];
      rects[i] = vpf_rect{(uint32_t)rois[i][1], (uint32_t)rois[i][2], (uint32_t)rois[i][3], (uint32_t)rois[i][4]};
    }
    return TASK_EXEC_SUCCESS == task_->RunTensorRois(a.data(), (uint32_t)a.size(), index.data(), rects.data(), (uint32_t)rois.size(), planes.data(), norm, cc.get());
  }
  // additive: up to max_n rectangles that lie in DEVICE memory -> a normalised planar tensor [max_n, 3, dh, dw] at device address `dst`
  // (vpf_convert_resize_tensor_rois_dev): entry k = five int32 (surface index, x, y, w, h) at boxes + k box_stride, *count (device int32; 0: max_n)
  // of them valid; read by the kernel when it runs on the task's stream.  At most 128 surfaces; tensor layout and mean / std as ExecuteToTensor
  bool ExecuteRoisDevToTensor(const std::vector<std::shared_ptr<Surface>>& src, uint64_t boxes, uint32_t max_n, uint64_t count, uint64_t dst, uint32_t dtype,
                              const std::vector<double>& mean, const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc, bool bgr,
                              uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride, bool channels_last, uint32_t box_stride) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (src.empty() || src.size() > 128 || !boxes || !max_n || !dst) return false;
    std::vector<vpf_plane> planes;  // two jobs' planes: the second minus the first is the stride from job to job
    if (!tensor_planes(dst, dtype, 2, task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    const uint64_t job_stride = (uint64_t)((uintptr_t)planes[channels_last ? 1 : 3].ptr - (uintptr_t)planes[0].ptr);
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    return TASK_EXEC_SUCCESS == task_->RunTensorRoisDev(a.data(), (uint32_t)a.size(), (const void*)(uintptr_t)boxes, box_stride, max_n,
                                                        (const void*)(uintptr_t)count, planes.data(), job_stride, norm, cc.get());
  }
  // additive: K affine warps of surfaces -> a normalised planar tensor [K, 3, dh, dw] at device address `dst` (vpf_convert_warp_tensor):
  // warps[i] = (surface index, m00, m01, m02, m10, m11, m12), the inverse matrix (destination pixel -> source luma pixel coordinates);
  // border per output channel, border_mode 0 = constant, 1 = replicate; tensor layout and mean / std as ExecuteToTensor
  bool ExecuteWarpsToTensor(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<int64_t>& index, const std::vector<std::array<float, 6>>& matrices,
                            uint64_t dst, uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std,
                            std::shared_ptr<ColorspaceConversionContext> cc, bool bgr, const std::array<int64_t, 3>& border, uint32_t border_mode,
                            uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride, bool channels_last) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (src.empty() || index.empty() || index.size() != matrices.size() || !dst) return false;
    std::vector<vpf_plane> planes;
    if (!tensor_planes(dst, dtype, index.size(), task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    vpf_warp_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.border_mode = border_mode;
    for (int c = 0; c < 3; c++) {
      if (border[c] < 0 || border[c] > 255) return false;
      opts.border[c] = (uint8_t)border[c];
    }
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    std::vector<uint32_t> idx(index.size());
    std::vector<float> m(6 * index.size());
    for (size_t i = 0; i < index.size(); i++) {
      if (index[i] < 0 || index[i] > 0xffffffffll) return false;
      idx[i] = (uint32_t)index[i];
      for (int k = 0; k < 6; k++) m[6 * i + k] = matrices[i][k];
    }
    return TASK_EXEC_SUCCESS == task_->RunTensorWarps(a.data(), (uint32_t)a.size(), idx.data(), m.data(), (uint32_t)index.size(), planes.data(), norm, &opts, cc.get());
  }
  // additive: K perspective warps of surfaces -> a normalised planar tensor [K, 3, dh, dw] at device address `dst` (vpf_convert_persp_tensor):
  // ExecuteWarpsToTensor with the inverse 3 x 3 matrix (nine floats, row-major) per job; a pixel with w <= 0 takes the border in both modes
  bool ExecutePerspsToTensor(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<int64_t>& index, const std::vector<std::array<float, 9>>& matrices,
                             uint64_t dst, uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std,
                             std::shared_ptr<ColorspaceConversionContext> cc, bool bgr, const std::array<int64_t, 3>& border, uint32_t border_mode,
                             uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride, bool channels_last) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (src.empty() || index.empty() || index.size() != matrices.size() || !dst) return false;
    std::vector<vpf_plane> planes;
    if (!tensor_planes(dst, dtype, index.size(), task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    vpf_warp_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.border_mode = border_mode;
    for (int c = 0; c < 3; c++) {
      if (border[c] < 0 || border[c] > 255) return false;
      opts.border[c] = (uint8_t)border[c];
    }
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    std::vector<uint32_t> idx(index.size());
    std::vector<float> m(9 * index.size());
    for (size_t i = 0; i < index.size(); i++) {
      if (index[i] < 0 || index[i] > 0xffffffffll) return false;
      idx[i] = (uint32_t)index[i];
      for (int k = 0; k < 9; k++) m[9 * i + k] = matrices[i][k];
    }
    return TASK_EXEC_SUCCESS == task_->RunTensorPersps(a.data(), (uint32_t)a.size(), idx.data(), m.data(), (uint32_t)index.size(), planes.data(), norm, &opts, cc.get());
  }
  // additive: up to max_n affine warps whose matrices lie in DEVICE memory -> a normalised planar tensor [max_n, 3, dh, dw] at device address `dst`
  // (vpf_convert_warp_tensor_dev): job k = six float32 at matrices + k matrix_stride, its surface index one int32 at index + k index_stride (index 0:
  // surface 0), *count (device int32; 0: max_n) of them valid; read by the kernel when it runs on the task's stream.  max_step: the LDS hint (0: none).
  // At most 128 surfaces; border, border_mode, tensor layout and mean / std as ExecuteWarpsToTensor
  bool ExecuteWarpsDevToTensor(const std::vector<std::shared_ptr<Surface>>& src, uint64_t matrices, uint32_t max_n, uint64_t index, uint64_t count, uint64_t dst,
                               uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc,
                               bool bgr, const std::array<int64_t, 3>& border, uint32_t border_mode, uint64_t row_pitch, uint64_t plane_stride,
                               uint64_t frame_stride, bool channels_last, uint32_t matrix_stride, uint32_t index_stride, float max_step) {
    return MatricesDevToTensor(false, src, matrices, max_n, index, count, dst, dtype, mean, std, cc, bgr, border, border_mode, row_pitch, plane_stride, frame_stride,
                               channels_last, matrix_stride, index_stride, max_step);
  }
  // additive: the same for perspective warps (vpf_convert_persp_tensor_dev): job k = nine float32 (m00 .. m22) at matrices + k matrix_stride; max_step: the
  // bound on the source pixels per destination pixel step (vpf_persp_max_step; 0: none).  Every other argument as ExecuteWarpsDevToTensor
  bool ExecutePerspsDevToTensor(const std::vector<std::shared_ptr<Surface>>& src, uint64_t matrices, uint32_t max_n, uint64_t index, uint64_t count, uint64_t dst,
                                uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc,
                                bool bgr, const std::array<int64_t, 3>& border, uint32_t border_mode, uint64_t row_pitch, uint64_t plane_stride,
                                uint64_t frame_stride, bool channels_last, uint32_t matrix_stride, uint32_t index_stride, float max_step) {
    return MatricesDevToTensor(true, src, matrices, max_n, index, count, dst, dtype, mean, std, cc, bgr, border, border_mode, row_pitch, plane_stride, frame_stride,
                               channels_last, matrix_stride, index_stride, max_step);
  }
  bool MatricesDevToTensor(bool persp, const std::vector<std::shared_ptr<Surface>>& src, uint64_t matrices, uint32_t max_n, uint64_t index, uint64_t count, uint64_t dst,
                           uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc,
                           bool bgr, const std::array<int64_t, 3>& border, uint32_t border_mode, uint64_t row_pitch, uint64_t plane_stride,
                           uint64_t frame_stride, bool channels_last, uint32_t matrix_stride, uint32_t index_stride, float max_step) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (src.empty() || src.size() > 128 || !matrices || !max_n || !dst) return false;
    std::vector<vpf_plane> planes;  // two jobs' planes: the second minus the first is the stride from job to job
    if (!tensor_planes(dst, dtype, 2, task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    const uint64_t job_stride = (uint64_t)((uintptr_t)planes[channels_last ? 1 : 3].ptr - (uintptr_t)planes[0].ptr);
    vpf_warp_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.border_mode = border_mode;
    for (int c = 0; c < 3; c++) {
      if (border[c] < 0 || border[c] > 255) return false;
      opts.border[c] = (uint8_t)border[c];
    }
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    const auto run = persp ? &ConvertResizeSurface::RunTensorPerspsDev : &ConvertResizeSurface::RunTensorWarpsDev;
    return TASK_EXEC_SUCCESS == ((*task_).*run)(a.data(), (uint32_t)a.size(), (const void*)(uintptr_t)matrices, matrix_stride, (const void*)(uintptr_t)index, index_stride,
                                                max_n, (const void*)(uintptr_t)count, max_step, planes.data(), job_stride, norm, &opts, cc.get());
  }
  // additive: K letterbox jobs -> a normalised planar tensor [K, 3, dh, dw] at device address `dst` (vpf_convert_letterbox_tensor): rois[i] as
  // ExecuteRoisToTensor, dst_rects[i] = (ix, iy, iw, ih) where that region's picture goes inside dw x dh, `pad` (per output channel) everywhere else;
  // std::invalid_argument (ValueError) for a pad value outside 0..255 and for rois / dst_rects of different lengths
  bool ExecuteLetterboxToTensor(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<std::array<int64_t, 5>>& rois,
                                const std::vector<std::array<int64_t, 4>>& dst_rects, uint64_t dst, uint32_t dtype, const std::vector<double>& mean,
                                const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc, bool bgr, const std::vector<int64_t>& pad,
                                uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride, bool channels_last) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (pad.size() != 3) throw std::invalid_argument("pad needs three values");
    vpf_letterbox_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    for (int c = 0; c < 3; c++) {
      if (pad[c] < 0 || pad[c] > 255) throw std::invalid_argument("pad values must lie in 0..255");
      opts.pad[c] = (uint8_t)pad[c];
    }
    if (rois.size() != dst_rects.size()) throw std::invalid_argument("rois and dst_rects must have the same length");
    if (src.empty() || rois.empty() || !dst) return false;
    std::vector<vpf_plane> planes;
    if (!tensor_planes(dst, dtype, rois.size(), task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    std::vector<uint32_t> index(rois.size());
    std::vector<vpf_rect> rects(rois.size()), drects(rois.size());
    for (size_t i = 0; i < rois.size(); i++) {
      for (int k = 0; k < 5; k++)
        if (rois[i][k] < 0 || rois[i][k] > 0xffffffffll) return false;
      for (int k = 0; k < 4; k++)
        if (dst_rects[i][k] < 0 || dst_rects[i][k] > 0xffffffffll) return false;
      index[i] = (uint32_t)rois[i][0];
      rects[i] = vpf_rect{(uint32_t)rois[i][1], (uint32_t)rois[i][2], (uint32_t)rois[i][3], (uint32_t)rois[i][4]};
      drects[i] = vpf_rect{(uint32_t)dst_rects[i][0], (uint32_t)dst_rects[i][1], (uint32_t)dst_rects[i][2], (uint32_t)dst_rects[i][3]};
    }
    return TASK_EXEC_SUCCESS == task_->RunTensorLetterbox(a.data(), (uint32_t)a.size(), index.data(), rects.data(), drects.data(), (uint32_t)rois.size(),
                                                          planes.data(), norm, &opts, cc.get());
  }
  // additive: the same jobs through the antialiasing triangle filter (vpf_convert_letterbox_tensor_aa): ExecuteLetterboxToTensor's arguments and answers
  bool ExecuteLetterboxAAToTensor(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<std::array<int64_t, 5>>& rois,
                                  const std::vector<std::array<int64_t, 4>>& dst_rects, uint64_t dst, uint32_t dtype, const std::vector<double>& mean,
                                  const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc, bool bgr, const std::vector<int64_t>& pad,
                                  uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride, bool channels_last) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (pad.size() != 3) throw std::invalid_argument("pad needs three values");
    vpf_letterbox_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    for (int c = 0; c < 3; c++) {
      if (pad[c] < 0 || pad[c] > 255) throw std::invalid_argument("pad values must lie in 0..255");
      opts.pad[c] = (uint8_t)pad[c];
    }
    if (rois.size() != dst_rects.size()) throw std::invalid_argument("rois and dst_rects must have the same length");
    if (src.empty() || rois.empty() || !dst) return false;
    std::vector<vpf_plane> planes;
    if (!tensor_planes(dst, dtype, rois.size(), task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    std::vector<uint32_t> index(rois.size());
    std::vector<vpf_rect> rects(rois.size()), drects(rois.size());
    for (size_t i = 0; i < rois.size(); i++) {
      for (int k = 0; k < 5; k++)
        if (rois[i][k] < 0 || rois[i][k] > 0xffffffffll) return false;
      for (int k = 0; k < 4; k++)
        if (dst_rects[i][k] < 0 || dst_rects[i][k] > 0xffffffffll) return false;
      index[i] = (uint32_t)rois[i][0];
      rects[i] = vpf_rect{(uint32_t)rois[i][1], (uint32_t)rois[i][2], (uint32_t)rois[i][3], (uint32_t)rois[i][4]};
      drects[i] = vpf_rect{(uint32_t)dst_rects[i][0], (uint32_t)dst_rects[i][1], (uint32_t)dst_rects[i][2], (uint32_t)dst_rects[i][3]};
    }
    return TASK_EXEC_SUCCESS == task_->RunTensorLetterboxAA(a.data(), (uint32_t)a.size(), index.data(), rects.data(), drects.data(), (uint32_t)rois.size(),
                                                            planes.data(), norm, &opts, cc.get());
  }
  // additive: up to max_n letterbox jobs whose boxes lie in DEVICE memory -> a normalised planar tensor [max_n, 3, dh, dw] at device address `dst`
  // (vpf_convert_letterbox_tensor_dev): ExecuteRoisDevToTensor's boxes and count, plus job k's placement, four int32 (ix, iy, iw, ih) at rects +
  // k rect_stride (rects 0: the kernel fits box k into dw x dh), `pad` (per output channel) wherever the frame shows no picture;
  // std::invalid_argument (ValueError) for a pad value outside 0..255
  bool ExecuteLetterboxDevToTensor(const std::vector<std::shared_ptr<Surface>>& src, uint64_t boxes, uint32_t max_n, uint64_t count, uint64_t rects,
                                   uint64_t dst, uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std,
                                   std::shared_ptr<ColorspaceConversionContext> cc, bool bgr, const std::vector<int64_t>& pad, uint64_t row_pitch,
                                   uint64_t plane_stride, uint64_t frame_stride, bool channels_last, uint32_t box_stride, uint32_t rect_stride) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (pad.size() != 3) throw std::invalid_argument("pad needs three values");
    vpf_letterbox_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    for (int c = 0; c < 3; c++) {
      if (pad[c] < 0 || pad[c] > 255) throw std::invalid_argument("pad values must lie in 0..255");
      opts.pad[c] = (uint8_t)pad[c];
    }
    if (src.empty() || src.size() > 128 || !boxes || !max_n || !dst) return false;
    std::vector<vpf_plane> planes;  // two jobs' planes: the second minus the first is the stride from job to job
    if (!tensor_planes(dst, dtype, 2, task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    const uint64_t job_stride = (uint64_t)((uintptr_t)planes[channels_last ? 1 : 3].ptr - (uintptr_t)planes[0].ptr);
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    return TASK_EXEC_SUCCESS == task_->RunTensorLetterboxDev(a.data(), (uint32_t)a.size(), (const void*)(uintptr_t)boxes, box_stride,
                                                             (const void*)(uintptr_t)rects, rect_stride, max_n, (const void*)(uintptr_t)count, planes.data(),
                                                             job_stride, norm, &opts, cc.get());
  }
  // additive: n surfaces, each through a per-pixel map pair -> a normalised planar tensor [n, 3, dh, dw] at device address `dst`
  // (vpf_convert_remap_tensor): frame i comes from src[i] through the float32 maps at xmap + i map_stride / ymap + i map_stride (DEVICE addresses;
  // map_stride 0: one pair for every frame; a pitch of 0: tight rows of dw floats), read by the kernel when it runs on the task's stream.  A NaN
  // coordinate takes the border in both modes.  max_step: the LDS hint (0: none).  border, border_mode, tensor layout and mean / std as
  // ExecuteWarpsToTensor
  bool ExecuteRemapToTensor(const std::vector<std::shared_ptr<Surface>>& src, uint64_t xmap, uint64_t ymap, uint64_t dst, uint32_t dtype,
                            const std::vector<double>& mean, const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc, bool bgr,
                            const std::array<int64_t, 3>& border, uint32_t border_mode, uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride,
                            bool channels_last, uint32_t xmap_pitch, uint32_t ymap_pitch, uint64_t map_stride, float max_step) {
    vpf_tensor_norm norm = norm_of(dtype, mean, std, bgr);
    if (src.empty() || !xmap || !ymap || !dst) return false;
    std::vector<vpf_plane> planes;
    if (!tensor_planes(dst, dtype, src.size(), task_dst_w_, task_dst_h_, row_pitch, plane_stride, frame_stride, channels_last, norm, planes)) return false;
    vpf_remap_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.border_mode = border_mode;
    opts.max_step = max_step;
    for (int c = 0; c < 3; c++) {
      if (border[c] < 0 || border[c] > 255) return false;
      opts.border[c] = (uint8_t)border[c];
    }
    std::vector<Surface*> a;
    for (auto& s : src) a.push_back(s.get());
    return TASK_EXEC_SUCCESS == task_->RunTensorRemap(a.data(), (uint32_t)a.size(), (const void*)(uintptr_t)xmap, xmap_pitch ? xmap_pitch : 4u * task_dst_w_,
                                                      (const void*)(uintptr_t)ymap, ymap_pitch ? ymap_pitch : 4u * task_dst_w_, map_stride, planes.data(), norm,
                                                      &opts, cc.get());
  }
  size_t GetStream() const { return (size_t)task_->GetStream(); }
  uint32_t task_dst_w_ = 0, task_dst_h_ = 0;
};

// additive: a planar float tensor [n, 3, H, W] (f32 / f16 / bf16) at a device address -> NV12 / YUV420 surfaces in one pass (TensorToSurface)
class PyTensorToSurface {
  std::unique_ptr<TensorToSurface> task_;
  Pixel_Format out_fmt_;
  uint32_t w_, h_;
  int dev_;

  // mean / std are the ones the tensor was normalised with (torchvision's, values of [0, 1] pixels), per input plane: scale = 255 std and
  // bias = 255 mean, computed in double and rounded to fp32
  static vpf_tensor_norm denorm_of(uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std, bool bgr) {
    if (mean.size() != 3 || std.size() != 3) throw std::invalid_argument("mean and std need three values each");
    vpf_tensor_norm d;
    std::memset(&d, 0, sizeof(d));
    for (int c = 0; c < 3; c++) {
      if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || !(std[c] > 0.0)) throw std::invalid_argument("mean must be finite and std finite and > 0");
      d.scale[c] = (float)(255.0 * std[c]);
      d.bias[c] = (float)(255.0 * mean[c]);
      if (!std::isfinite(d.scale[c]) || !std::isfinite(d.bias[c])) throw std::invalid_argument("mean / std give a scale or bias beyond fp32");
    }
    d.dtype = dtype;
    d.flags = bgr ? VPF_TENSOR_BGR : 0u;
    return d;
  }
  // element (i, c, y, x) at src + i frame_stride + c plane_stride + y row_pitch + x elem (bytes; 0 = contiguous NCHW); channels_last: tensor_planes
  bool planes_of(uint64_t src, uint32_t dtype, size_t n, uint64_t row_pitch, uint64_t plane_stride, uint64_t frame_stride, bool channels_last,
                 vpf_tensor_norm& d, std::vector<vpf_plane>& planes) const {
    if (!src || !n) return false;
    return tensor_planes(src, dtype, n, w_, h_, row_pitch, plane_stride, frame_stride, channels_last, d, planes);
  }

public:
  PyTensorToSurface(uint32_t w, uint32_t h, Pixel_Format out, HipContext ctx, HipStream str) : out_fmt_(out), w_(w), h_(h), dev_(DeviceOfContext(ctx)) {
    task_.reset(TensorToSurface::Make(w, h, out, ctx, str));
  }
  int Device() const { return dev_; }  // the GPU the converter was built for; -1: whatever device is current
  Pixel_Format GetFormat() const { return out_fmt_; }
  size_t GetStream() const { return (size_t)task_->GetStream(); }
  uint32_t Width() const { return w_; }
  uint32_t Height() const { return h_; }
  // one frame [3, H, W] -> a NON-OWNING alias of the task's single output surface (overwritten by the next Execute); failure = Empty()
  std::shared_ptr<Surface> Execute(uint64_t src, uint32_t dtype, const std::vector<double>& mean, const std::vector<double>& std,
                                   std::shared_ptr<ColorspaceConversionContext> cc, bool bgr, uint64_t row_pitch, uint64_t plane_stride,
                                   bool channels_last) {
    vpf_tensor_norm d = denorm_of(dtype, mean, std, bgr);
    std::vector<vpf_plane> planes;
    if (!planes_of(src, dtype, 1, row_pitch, plane_stride, 0, channels_last, d, planes)) return empty_surface(out_fmt_);
    planes.resize(3);  // (RunTensor takes src[3]; channels_last reads src[0] only)
    Surface* out = task_->RunTensor(planes.data(), d, cc.get());
    return out ? std::shared_ptr<Surface>(out->Clone()) : empty_surface(out_fmt_);
  }
  // frames [len(dst), 3, H, W] -> the caller's surfaces, one dispatch per 32 frames
  bool ExecuteBatch(uint64_t src, const std::vector<std::shared_ptr<Surface>>& dst, uint32_t dtype, const std::vector<double>& mean,
                    const std::vector<double>& std, std::shared_ptr<ColorspaceConversionContext> cc, bool bgr, uint64_t row_pitch,
                    uint64_t plane_stride, uint64_t frame_stride, bool channels_last) {
    vpf_tensor_norm d = denorm_of(dtype, mean, std, bgr);
    std::vector<vpf_plane> planes;
    if (!planes_of(src, dtype, dst.size(), row_pitch, plane_stride, frame_stride, channels_last, d, planes)) return false;
    std::vector<Surface*> b;
    for (auto& s : dst) b.push_back(s.get());
    return TASK_EXEC_SUCCESS == task_->RunTensorBatch(planes.data(), b.data(), (uint32_t)b.size(), d, cc.get());
  }
};

class PySurfaceResizer {
  std::unique_ptr<ResizeSurface> rs_;
  Pixel_Format fmt_;

public:
  PySurfaceResizer(uint32_t w, uint32_t h, Pixel_Format f, HipContext ctx, HipStream str) : fmt_(f) {
    rs_.reset(ResizeSurface::Make(w, h, f, ctx, str));
  }
  Pixel_Format GetFormat() const { return fmt_; }
  void SetInterpolation(int i) { rs_->SetInterpolation(i); }
  void SetAsync(bool on) { rs_->SetAsync(on); }
  bool GetAsync() const { return rs_->GetAsync(); }
  int GetInterpolation() const { return rs_->GetInterpolation(); }
  std::shared_ptr<Surface> Execute(std::shared_ptr<Surface> src) {
    if (!src) return empty_surface(fmt_);
    rs_->SetInput(src.get(), 0U);
    if (TASK_EXEC_SUCCESS != rs_->Execute()) return empty_surface(fmt_);
    auto* out = static_cast<Surface*>(rs_->GetOutput(0U));
    return std::shared_ptr<Surface>(out ? out->Clone() : Surface::Make(fmt_));
  }
  // additive: n surfaces in, n caller-owned surfaces out, every plane of every frame in as few dispatches as possible
  bool ExecuteBatch(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<std::shared_ptr<Surface>>& dst) {
    if (src.size() != dst.size() || src.empty()) return false;
    std::vector<Surface*> a, b;
    for (auto& s : src) a.push_back(s.get());
    for (auto& d : dst) b.push_back(d.get());
    return TASK_EXEC_SUCCESS == rs_->RunBatch(a.data(), b.data(), (uint32_t)a.size());
  }
};

class PySurfaceRemaper {
  std::unique_ptr<RemapSurface> rm_;
  Pixel_Format fmt_;

public:
  PySurfaceRemaper(py::array_t<float, py::array::c_style | py::array::forcecast>& x, py::array_t<float, py::array::c_style | py::array::forcecast>& y,
                   Pixel_Format f, HipContext ctx, HipStream str)
      : fmt_(f) {
    if (x.ndim() != 2 || y.ndim() != 2 || x.shape(0) != y.shape(0) || x.shape(1) != y.shape(1))
      throw std::runtime_error("x_map and y_map must be 2-D float32 arrays of the same shape");
    rm_.reset(RemapSurface::Make(x.data(), y.data(), (uint32_t)x.shape(1), (uint32_t)x.shape(0), f, ctx, str));
  }
  Pixel_Format GetFormat() const { return fmt_; }
  void SetAsync(bool on) { rm_->SetAsync(on); }
  bool GetAsync() const { return rm_->GetAsync(); }
  std::shared_ptr<Surface> Execute(std::shared_ptr<Surface> src) {
    if (!src) return empty_surface(fmt_);
    rm_->SetInput(src.get(), 0U);
    if (TASK_EXEC_SUCCESS != rm_->Execute()) return empty_surface(fmt_);
    auto* out = static_cast<Surface*>(rm_->GetOutput(0U));
    return std::shared_ptr<Surface>(out ? out->Clone() : Surface::Make(fmt_));
  }
  // additive: the same maps applied to n surfaces into n caller-owned surfaces, one dispatch per 32 frames
  bool ExecuteBatch(const std::vector<std::shared_ptr<Surface>>& src, const std::vector<std::shared_ptr<Surface>>& dst) {
    if (src.size() != dst.size() || src.empty()) return false;
    std::vector<Surface*> a, b;
    for (auto& s : src) a.push_back(s.get());
    for (auto& d : dst) b.push_back(d.get());
    return TASK_EXEC_SUCCESS == rm_->RunBatch(a.data(), b.data(), (uint32_t)a.size());
  }
};

// The numpy array that OWNS a frame's memory (the end of the .base chain), if the frame is a plain view of it: the object HostPinCache may
// key a page-locked registration on — its death (a weak-reference callback) is when the memory can go away.  nullptr: nobody to vouch for the
// memory (a bytes / bytearray / mmap / foreign buffer at the root, an array that does not own its data): the upload stages a copy as before.
static PyObject* frame_owner(const py::array& f) {
  py::handle o = f;
  for (int depth = 0; depth < 8; depth++) {
    if (!py::isinstance<py::array>(o)) return nullptr;
    py::object base = py::reinterpret_borrow<py::array>(o).base();
    if (!base || base.is_none()) return py::reinterpret_borrow<py::array>(o).owndata() ? o.ptr() : nullptr;
    o = base;  // (borrowed: the chain is kept alive by `f` for the duration of the call)
    if (py::isinstance<py::capsule>(o)) return nullptr;  // AllocPinned(): page-locked already
  }
  return nullptr;
}
// Does the buffer own its PAGES?  hipHostRegister / hipHostUnregister work on whole pages, and unregistering tears the GPU mapping of every page of
// the range down — also for whatever else lives in the range's first and last page.  The HIP runtime page-locks pageable memory on the fly for its
// own copies (torch's .cpu(), hipMemcpy from a numpy array) and keeps track of what it has locked: when a buffer this cache releases shares a page
// with memory the runtime believes locked, the runtime's next copy there faults on the GPU ("Memory access fault by GPU ... on address <host page>":
// seen in 3 of 19 long single-process test runs, profiles/r06_pin_cache_fault.txt).  So only buffers that own their pages are taken: glibc serves
// large requests by mmap — a chunk of whole pages of its own, user pointer 16 bytes in, IS_MMAPPED set in the size word in front of it (read only
// when the pointer sits 16 bytes into a page: the word is then on the same, mapped, page).  Heap-cut buffers keep the staged copy.
static bool owns_its_pages(const void* data, size_t bytes) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(data);
  if ((p & 4095u) != 16u) return false;
  const size_t word = reinterpret_cast<const size_t*>(p)[-1], chunk = word & ~(size_t)7;
  return (word & 2u) != 0 && (chunk & 4095u) == 0 && chunk >= bytes + 16u;
}
static void vouch_for_frame(const py::array& f, const void* data, size_t bytes, int device) {
  if (!owns_its_pages(data, bytes)) return;
  PyObject* owner = frame_owner(f);
  if (!owner) return;
  const uint64_t id = (uint64_t)(uintptr_t)owner;
  if (HostPinCache::note_use(data, bytes, id, device) != HostPinCache::kFirstSight) return;
  // the owner's first buffer: from now on its death unregisters whatever was page-locked on its behalf (before numpy frees the memory:
  // weak-reference callbacks run before tp_dealloc releases the data)
  py::weakref(py::handle(owner), py::cpp_function([id](py::handle wr) {
                HostPinCache::owner_gone(id);
                wr.dec_ref();
              })).release();
}

class PyFrameUploader {
  std::unique_ptr<CudaUploadFrame> up_;
  Pixel_Format fmt_;
  int dev_ = 0;

public:
  PyFrameUploader(uint32_t w, uint32_t h, Pixel_Format f, HipContext ctx, HipStream str) : fmt_(f) {
    up_.reset(CudaUploadFrame::Make(str, ctx, w, h, f));
    dev_ = DeviceOfContext(ctx);  // (-1: whatever device is current)
  }
  Pixel_Format GetFormat() const { return fmt_; }
  int Device() const { return dev_; }
  void SetAsync(bool on, bool in_place) { up_->SetAsync(on); up_->SetAsyncInPlace(on && in_place); }
  bool GetAsync() const { return up_->GetAsync(); }
  bool Vouches() const { return !up_->GetAsync() || up_->GetAsyncInPlace(); }  // uploads that may read a caller frame in place: blocking ones, asynchronous ones on the caller's promise
  std::shared_ptr<Surface> Upload(void* data, size_t bytes) {
    py::gil_scoped_release nogil;  // the reference releases the GIL around uploads too (PyFrameUploader.cpp:118-160)
    std::unique_ptr<Buffer> raw(Buffer::Make(bytes, data));
    up_->SetInput(raw.get(), 0U);
    const auto res = up_->Execute();
    up_->ClearInputs();
    auto* s = static_cast<Surface*>(up_->GetOutput(0U));
    if (TASK_EXEC_FAIL == res || !s) throw std::runtime_error("Error uploading frame to GPU");
    return std::shared_ptr<Surface>(s->Clone());
  }
};

class PySurfaceDownloader {
  std::unique_ptr<CudaDownloadSurface> dl_;
  Pixel_Format fmt_;

public:
  PySurfaceDownloader(uint32_t w, uint32_t h, Pixel_Format f, HipContext ctx, HipStream str) : fmt_(f) {
    dl_.reset(CudaDownloadSurface::Make(str, ctx, w, h, f));
  }
  Pixel_Format GetFormat() const { return fmt_; }
  template <typename T>
  bool Download(std::shared_ptr<Surface> s, py::array_t<T>& frame) {
    if (!s || s->Empty()) return false;
    const size_t bytes = s->HostMemSize();
    if (bytes != (size_t)frame.size() * sizeof(T)) frame.resize({(py::ssize_t)(bytes / sizeof(T))}, false);
    T* dst = frame.mutable_data();
    // the DMA and (for pageable arrays) the single host copy run without the GIL; arrays from AllocPinned() receive
    // the DMA directly
    py::gil_scoped_release nogil;
    return TASK_EXEC_SUCCESS == dl_->DownloadInto(s.get(), dst, bytes);
  }
};

class PyBufferUploader {
  std::unique_ptr<UploadBuffer> up_;

public:
  PyBufferUploader(uint32_t e, uint32_t n, HipContext ctx, HipStream str) { up_.reset(UploadBuffer::Make(str, ctx, e, n)); }
  std::shared_ptr<CudaBuffer> Upload(py::array_t<uint8_t>& a) {
    std::unique_ptr<Buffer> raw(Buffer::Make((size_t)a.size(), a.mutable_data()));
    up_->SetInput(raw.get(), 0U);
    const auto res = up_->Execute();
    up_->ClearInputs();
    auto* b = static_cast<CudaBuffer*>(up_->GetOutput(0U));
    if (TASK_EXEC_FAIL == res || !b) throw std::runtime_error("Error uploading frame to GPU");
    return std::shared_ptr<CudaBuffer>(b->Clone());
  }
};

class PyCudaBufferDownloader {
  std::unique_ptr<DownloadCudaBuffer> dl_;

public:
  PyCudaBufferDownloader(uint32_t e, uint32_t n, HipContext ctx, HipStream str) { dl_.reset(DownloadCudaBuffer::Make(str, ctx, e, n)); }
  bool Download(std::shared_ptr<CudaBuffer> b, py::array_t<uint8_t>& a) {
    if (!b) return false;
    dl_->SetInput(b.get(), 0U);
    if (TASK_EXEC_FAIL == dl_->Execute()) return false;
    auto* raw = static_cast<Buffer*>(dl_->GetOutput(0U));
    if (!raw) return false;
    const size_t bytes = b->GetRawMemSize();
    if (bytes != (size_t)a.size()) a.resize({(py::ssize_t)bytes}, false);
    std::memcpy(a.mutable_data(), raw->GetRawMemPtr(), bytes);
    return true;
  }
};
#ifdef VPF_WITH_LIBAV
// PyFfmpegDecoder (reference: src/PyNvCodec/src/PyFFMpegDecoder.cpp:37-70,220-268): software decode on the host, frames
// enter the GPU through the pinned-staging uploader.  Only compiled where libav exists.
class PyFfmpegDecoder {
  std::unique_ptr<FfmpegFeeder> dec_;
  std::unique_ptr<PyFrameUploader> up_;
  std::vector<uint8_t> host_;
  int gpu_;

public:
  PyFfmpegDecoder(const std::string& url, const std::map<std::string, std::string>& opts, int gpu) : gpu_(gpu) {
    dec_.reset(new FfmpegFeeder(url, opts));
  }
  uint32_t Width() const { return dec_->Width(); }
  uint32_t Height() const { return dec_->Height(); }
  double Framerate() const { return dec_->Framerate(); }
  ColorSpace GetColorSpace() const { return dec_->GetColorSpace(); }
  ColorRange GetColorRange() const { return dec_->GetColorRange(); }
  Pixel_Format GetPixelFormat() const { return dec_->GetPixelFormat(); }
  uint32_t up_w_ = 0, up_h_ = 0;
  // uploaders of earlier resolutions, keyed by size: surfaces already handed out alias their memory, and a stream that alternates between
  // resolutions gets its old uploader back instead of a new pair of pinned + device buffers per switch
  std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<PyFrameUploader>> parked_;

  bool DecodeSingleFrame(py::array_t<uint8_t>& frame) {
    if (!dec_->NextFrame()) return false;
    const size_t n = dec_->PendingFrameBytes();  // sized from the decoded picture: a stream may change resolution mid-way
    if ((size_t)frame.size() != n) frame.resize({(py::ssize_t)n}, false);
    return dec_->CopyFrameNV12(frame.mutable_data(), n);
  }
  std::shared_ptr<Surface> DecodeSingleSurface() {
    if (!dec_->NextFrame()) return empty_surface(NV12);
    const uint32_t w = dec_->FrameWidth(), h = dec_->FrameHeight();
    host_.resize(dec_->PendingFrameBytes());
    if (!dec_->CopyFrameNV12(host_.data(), host_.size())) return empty_surface(NV12);
    if (!up_ || w != up_w_ || h != up_h_) {
      if (up_) parked_[{up_w_, up_h_}] = std::move(up_);
      auto it = parked_.find({w, h});
      if (it != parked_.end()) { up_ = std::move(it->second); parked_.erase(it); }
      else up_.reset(new PyFrameUploader(w, h, NV12, ctx_of(gpu_), str_of(gpu_)));
      up_w_ = w; up_h_ = h;
    }
    return up_->Upload(host_.data(), host_.size());
  }
};
#endif

}  // namespace

PYBIND11_MODULE(_PyNvCodec, m) {
  m.doc() = "MI355X-native surface conversion behind VPF's Python API (hand-written HIP kernels via libvpfhip)";

  py::enum_<Pixel_Format>(m, "PixelFormat")
      .value("Y", Y).value("RGB", RGB).value("NV12", NV12).value("YUV420", YUV420).value("RGB_PLANAR", RGB_PLANAR)
      .value("BGR", BGR).value("YCBCR", YCBCR).value("YUV444", YUV444).value("YUV444_10bit", YUV444_10bit)
      .value("YUV420_10bit", YUV420_10bit).value("UNDEFINED", UNDEFINED).value("RGB_32F", RGB_32F)
      .value("RGB_32F_PLANAR", RGB_32F_PLANAR).value("YUV422", YUV422).value("P10", P10).value("P12", P12)
      .export_values();
  py::enum_<ColorSpace>(m, "ColorSpace").value("BT_601", BT_601).value("BT_709", BT_709).value("UNSPEC", UNSPEC).export_values();
  py::enum_<ColorRange>(m, "ColorRange").value("MPEG", MPEG).value("JPEG", JPEG).value("UDEF", UDEF).export_values();

  py::class_<ColorspaceConversionContext, std::shared_ptr<ColorspaceConversionContext>>(m, "ColorspaceConversionContext")
      .def(py::init<>())
      .def(py::init<ColorSpace, ColorRange>(), py::arg("color_space"), py::arg("color_range"))
      .def_readwrite("color_space", &ColorspaceConversionContext::color_space)
      .def_readwrite("color_range", &ColorspaceConversionContext::color_range);

  py::class_<CudaBuffer, std::shared_ptr<CudaBuffer>>(m, "CudaBuffer")
      .def("GetRawMemSize", &CudaBuffer::GetRawMemSize)
      .def("GetNumElems", &CudaBuffer::GetNumElems)
      .def("GetElemSize", &CudaBuffer::GetElemSize)
      .def("GpuMem", &CudaBuffer::GpuMem)
      .def("Clone", [](std::shared_ptr<CudaBuffer> self) { return std::shared_ptr<CudaBuffer>(self->Clone()); })
      .def("CopyFrom",
           [](std::shared_ptr<CudaBuffer> self, std::shared_ptr<CudaBuffer> other, size_t ctx, size_t str) {
             if (self->GetRawMemSize() != other->GetRawMemSize()) throw std::runtime_error("Buffers have different size.");
             std::unique_ptr<SurfacePlane> d(new SurfacePlane((uint32_t)self->GetRawMemSize(), 1, (uint32_t)self->GetRawMemSize(), 1, self->GpuMem()));
             d->Import(other->GpuMem(), (uint32_t)other->GetRawMemSize(), (HipContext)ctx, (HipStream)str);
           },
           py::arg("other"), py::arg("context"), py::arg("stream"))
      .def("CopyFrom",
           [](std::shared_ptr<CudaBuffer> self, std::shared_ptr<CudaBuffer> other, int gpu) {
             if (self->GetRawMemSize() != other->GetRawMemSize()) throw std::runtime_error("Buffers have different size.");
             std::unique_ptr<SurfacePlane> d(new SurfacePlane((uint32_t)self->GetRawMemSize(), 1, (uint32_t)self->GetRawMemSize(), 1, self->GpuMem()));
             d->Import(other->GpuMem(), (uint32_t)other->GetRawMemSize(), ctx_of(gpu), str_of(gpu));
           },
           py::arg("other"), py::arg("gpu_id"))
      .def_static("Make", [](uint32_t e, uint32_t n, int gpu) { return std::shared_ptr<CudaBuffer>(CudaBuffer::Make(e, n, ctx_of(gpu))); },
                  py::arg("elem_size"), py::arg("num_elems"), py::arg("gpu_id"));

  py::class_<SurfacePlane, std::shared_ptr<SurfacePlane>>(m, "SurfacePlane")
      .def("Width", &SurfacePlane::Width)
      .def("Height", &SurfacePlane::Height)
      .def("Pitch", &SurfacePlane::Pitch)
      .def("GpuMem", &SurfacePlane::GpuMem)
      .def("ElemSize", &SurfacePlane::ElemSize)
      .def("HostFrameSize", &SurfacePlane::GetHostMemSize)
      .def("Import", [](std::shared_ptr<SurfacePlane> self, size_t src, uint32_t pitch, int gpu) { self->Import((DevicePtr)src, pitch, ctx_of(gpu), str_of(gpu)); },
           py::arg("src"), py::arg("src_pitch"), py::arg("gpu_id"))
      .def("Import", [](std::shared_ptr<SurfacePlane> self, size_t src, uint32_t pitch, size_t ctx, size_t str) { self->Import((DevicePtr)src, pitch, (HipContext)ctx, (HipStream)str); },
           py::arg("src"), py::arg("src_pitch"), py::arg("context"), py::arg("stream"))
      .def("Export", [](std::shared_ptr<SurfacePlane> self, size_t dst, uint32_t pitch, int gpu) { self->Export((DevicePtr)dst, pitch, ctx_of(gpu), str_of(gpu)); },
           py::arg("dst"), py::arg("dst_pitch"), py::arg("gpu_id"))
      .def("Export", [](std::shared_ptr<SurfacePlane> self, size_t dst, uint32_t pitch, size_t ctx, size_t str) { self->Export((DevicePtr)dst, pitch, (HipContext)ctx, (HipStream)str); },
           py::arg("dst"), py::arg("dst_pitch"), py::arg("context"), py::arg("stream"))
      .def("__repr__", [](std::shared_ptr<SurfacePlane> self) { return plane_repr(self.get()); });

  py::class_<Surface, std::shared_ptr<Surface>>(m, "Surface", py::dynamic_attr())
      // additive: non-owning Surface over memory someone else owns (a torch tensor, a decoder's frame pool); the
      // reference has the equivalent only in C++ (SurfaceNV12(width, height, pitch, ptr), MemoryInterfaces.cpp:822-826)
      .def_static("Wrap",
                  [](Pixel_Format f, uint32_t w, uint32_t h, uint32_t pitch, size_t ptr) {
                    Surface* s = Surface::Make(f, w, h, pitch, (DevicePtr)ptr);
                    if (!s) throw std::invalid_argument("Surface.Wrap: format must live in ONE pitched allocation (Y, NV12, P10, P12, RGB, BGR, RGB_PLANAR, YUV444, RGB_32F, RGB_32F_PLANAR)");
                    return std::shared_ptr<Surface>(s);
                  },
                  py::arg("format"), py::arg("width"), py::arg("height"), py::arg("pitch"), py::arg("ptr"))
      .def("Width", &Surface::Width, py::arg("plane") = 0U)
      .def("Height", &Surface::Height, py::arg("plane") = 0U)
      .def("Pitch", &Surface::Pitch, py::arg("plane") = 0U)
      .def("Format", &Surface::PixelFormat)
      .def("Empty", &Surface::Empty)
      .def("NumPlanes", &Surface::NumPlanes)
      .def("HostSize", &Surface::HostMemSize)
      .def("OwnMemory", &Surface::OwnMemory)
      .def_static("Make", [](Pixel_Format f, uint32_t w, uint32_t h, int gpu) { return make_surface(f, w, h, ctx_of(gpu)); },
                  py::arg("format"), py::arg("width"), py::arg("height"), py::arg("gpu_id"))
      .def_static("Make", [](Pixel_Format f, uint32_t w, uint32_t h, size_t ctx) { return make_surface(f, w, h, (HipContext)ctx); },
                  py::arg("format"), py::arg("width"), py::arg("height"), py::arg("context"))
      .def("PlanePtr",
           [](std::shared_ptr<Surface> self, int plane) {
             SurfacePlane* p = self->GetSurfacePlane((uint32_t)plane);
             if (!p) throw std::invalid_argument("Invalid plane number");
             return std::make_shared<SurfacePlane>(*p);  // non-owning copy
           },
           py::arg("plane") = 0U)
      // Drop-in semantics: the reference's binding copies SELF -> OTHER (PySurface.cpp:54-81 takes (self, other) as (source,
      // destination) and :361,382 pass them in that order) — the opposite of what the name suggests, but code written against the
      // reference relies on it, so it is kept.  UpdateFrom (additive) is the unambiguous other -> self copy.
      .def("CopyFrom",
           [](std::shared_ptr<Surface> self, std::shared_ptr<Surface> other, int gpu) {
             check_same(*self, *other);
             copy_surface(*self, *other, ctx_of(gpu), str_of(gpu));
           },
           py::arg("other"), py::arg("gpu_id"), "DtoD copy of THIS surface INTO `other` (the reference's direction, PySurface.cpp:361)")
      .def("CopyFrom",
           [](std::shared_ptr<Surface> self, std::shared_ptr<Surface> other, size_t ctx, size_t str) {
             check_same(*self, *other);
             copy_surface(*self, *other, (HipContext)ctx, (HipStream)str);
           },
           py::arg("other"), py::arg("context"), py::arg("stream"), "DtoD copy of THIS surface INTO `other` (the reference's direction, PySurface.cpp:382)")
      .def("UpdateFrom",
           [](std::shared_ptr<Surface> self, std::shared_ptr<Surface> src, int gpu) {
             check_same(*self, *src);
             copy_surface(*src, *self, ctx_of(gpu), str_of(gpu));
           },
           py::arg("src"), py::arg("gpu_id"), "additive: DtoD copy of `src` into THIS surface")
      .def("UpdateFrom",
           [](std::shared_ptr<Surface> self, std::shared_ptr<Surface> src, size_t ctx, size_t str) {
             check_same(*self, *src);
             copy_surface(*src, *self, (HipContext)ctx, (HipStream)str);
           },
           py::arg("src"), py::arg("context"), py::arg("stream"), "additive: DtoD copy of `src` into THIS surface")
      .def("Clone",
           [](std::shared_ptr<Surface> self) {
             auto n = make_surface(self->PixelFormat(), self->Width(), self->Height(), self->Context());
             copy_surface(*self, *n, self->Context(), nullptr);
             return n;
           },
           py::call_guard<py::gil_scoped_release>())
      .def("Clone",
           [](std::shared_ptr<Surface> self, int gpu) {
             auto n = make_surface(self->PixelFormat(), self->Width(), self->Height(), ctx_of(gpu));
             copy_surface(*self, *n, ctx_of(gpu), str_of(gpu));
             return n;
           },
           py::arg("gpu_id"), py::call_guard<py::gil_scoped_release>())
      .def("Clone",
           [](std::shared_ptr<Surface> self, size_t ctx, size_t str) {
             auto n = make_surface(self->PixelFormat(), self->Width(), self->Height(), (HipContext)ctx);
             copy_surface(*self, *n, (HipContext)ctx, (HipStream)str);
             return n;
           },
           py::arg("context"), py::arg("stream"), py::call_guard<py::gil_scoped_release>())
      .def("Crop",
           [](std::shared_ptr<Surface> self, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int gpu) {
             auto n = make_surface(self->PixelFormat(), w, h, ctx_of(gpu));
             self->Export(*n, ctx_of(gpu), str_of(gpu), x, y, w, h, 0U, 0U);
             return n;
           },
           py::arg("x"), py::arg("y"), py::arg("w"), py::arg("h"), py::arg("gpu_id"), py::call_guard<py::gil_scoped_release>())
      .def("Crop",
           [](std::shared_ptr<Surface> self, uint32_t x, uint32_t y, uint32_t w, uint32_t h, size_t ctx, size_t str) {
             auto n = make_surface(self->PixelFormat(), w, h, (HipContext)ctx);
             self->Export(*n, (HipContext)ctx, (HipStream)str, x, y, w, h, 0U, 0U);
             return n;
           },
           py::arg("x"), py::arg("y"), py::arg("w"), py::arg("h"), py::arg("context"), py::arg("stream"),
           py::call_guard<py::gil_scoped_release>())
      .def("__repr__", [](std::shared_ptr<Surface> self) { return surface_repr(self.get()); });

  py::class_<PySurfaceConverter>(m, "PySurfaceConverter")
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format in, Pixel_Format out, uint32_t gpu) {
             return new PySurfaceConverter(w, h, in, out, ctx_of((int)gpu), str_of((int)gpu));
           }),
           py::arg("width"), py::arg("height"), py::arg("src_format"), py::arg("dst_format"), py::arg("gpu_id"))
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format in, Pixel_Format out, size_t ctx, size_t str) {
             return new PySurfaceConverter(w, h, in, out, (HipContext)ctx, (HipStream)str);
           }),
           py::arg("width"), py::arg("height"), py::arg("src_format"), py::arg("dst_format"), py::arg("context"), py::arg("stream"))
      .def("Format", &PySurfaceConverter::GetFormat)
      .def("SetOutputReuseHint", &PySurfaceConverter::SetOutputReuseHint, py::arg("on"),
           "additive: the result is consumed by the next kernel of a per-frame chain -> keep it in the Infinity Cache (identical pixels)")
      .def("GetOutputReuseHint", &PySurfaceConverter::GetOutputReuseHint)
      // the returned Surface aliases memory owned by the converter: keep the converter alive as long as it lives
      .def("Execute", &PySurfaceConverter::Execute, py::arg("src"), py::arg("cc_ctx") = nullptr, py::keep_alive<0, 1>(),
           py::call_guard<py::gil_scoped_release>())
      .def("ExecuteBatch", &PySurfaceConverter::ExecuteBatch, py::arg("src"), py::arg("dst"), py::arg("cc_ctx") = nullptr,
           py::call_guard<py::gil_scoped_release>());

  py::class_<PySurfaceConvertResizer>(m, "PySurfaceConvertResizer",
                                      "Additive: NV12 / YUV420 -> bilinear resize -> RGB / BGR / RGB_PLANAR in one pass; bit-identical to "
                                      "PySurfaceConverter followed by PySurfaceResizer (bilinear).  P10 / P12 sources construct too, for ExecuteToTensor / "
                                      "ExecuteRoisToTensor / ExecuteWarpsToTensor only: every 16-bit sample is narrowed to min(255, (v + 128) >> 8) (the bytes of "
                                      "PySurfaceConverter P10 -> NV12) at the load, then NV12's path; Execute / ExecuteBatch of such an instance refuse (Empty() "
                                      "surface / False, with a message): the 8-bit outputs take 8-bit sources.")
      .def(py::init([](uint32_t sw, uint32_t sh, Pixel_Format in, uint32_t dw, uint32_t dh, Pixel_Format out, uint32_t gpu) {
             return new PySurfaceConvertResizer(sw, sh, in, dw, dh, out, ctx_of((int)gpu), str_of((int)gpu));
           }),
           py::arg("src_width"), py::arg("src_height"), py::arg("src_format"), py::arg("dst_width"), py::arg("dst_height"),
           py::arg("dst_format"), py::arg("gpu_id"))
      .def(py::init([](uint32_t sw, uint32_t sh, Pixel_Format in, uint32_t dw, uint32_t dh, Pixel_Format out, size_t ctx, size_t str) {
             return new PySurfaceConvertResizer(sw, sh, in, dw, dh, out, (HipContext)ctx, (HipStream)str);
           }),
           py::arg("src_width"), py::arg("src_height"), py::arg("src_format"), py::arg("dst_width"), py::arg("dst_height"),
           py::arg("dst_format"), py::arg("context"), py::arg("stream"))
      .def("Format", &PySurfaceConvertResizer::GetFormat)
      .def("Execute", &PySurfaceConvertResizer::Execute, py::arg("src"), py::arg("cc_ctx") = nullptr, py::keep_alive<0, 1>(),
           py::call_guard<py::gil_scoped_release>())
      .def("ExecuteBatch", &PySurfaceConvertResizer::ExecuteBatch, py::arg("src"), py::arg("dst"), py::arg("cc_ctx") = nullptr,
           py::call_guard<py::gil_scoped_release>())
      .def("ExecuteToTensor", &PySurfaceConvertResizer::ExecuteToTensor, py::arg("src"), py::arg("dst"), py::arg("dtype"), py::arg("mean"),
           py::arg("std"), py::arg("cc_ctx") = nullptr, py::arg("bgr") = false, py::arg("row_pitch") = 0, py::arg("plane_stride") = 0,
           py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::call_guard<py::gil_scoped_release>())
      .def("ExecuteRoisToTensor", &PySurfaceConvertResizer::ExecuteRoisToTensor, py::arg("surfaces"), py::arg("rois"), py::arg("ptr"), py::arg("dtype"),
           py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr, py::arg("bgr") = false, py::arg("row_stride") = 0, py::arg("plane_stride") = 0,
           py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::call_guard<py::gil_scoped_release>(),
           "K rectangles (surface_index, x, y, w, h) of the surfaces, each resized to the task's destination size and normalised, into a planar tensor "
           "[K, 3, dh, dw] at device address ptr (strides in bytes, 0 = contiguous); one dispatch per 96 regions")
      .def("ExecuteRoisDevToTensor", &PySurfaceConvertResizer::ExecuteRoisDevToTensor, py::arg("surfaces"), py::arg("boxes_ptr"), py::arg("max_n"),
           py::arg("count_ptr"), py::arg("ptr"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr, py::arg("bgr") = false,
           py::arg("row_stride") = 0, py::arg("plane_stride") = 0, py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::arg("box_stride") = 20u,
           py::call_guard<py::gil_scoped_release>(),
           "Up to max_n rectangles that lie in DEVICE memory: entry k = five int32 (surface_index, x, y, w, h) at boxes_ptr + k box_stride, the first "
           "*count_ptr (a device int32; 0 = max_n) of them resized to the task's destination size and normalised into frame k of a planar tensor "
           "[max_n, 3, dh, dw] at device address ptr (strides in bytes, 0 = contiguous).  The kernel reads boxes and count when it runs on the task's "
           "stream: no sync, no copy to the host, capturable.  An invalid box gives a frame of normalised zeros; frames at or behind the count are "
           "not written.  At most 128 surfaces; one dispatch")
      .def("ExecutePerspsDevToTensor", &PySurfaceConvertResizer::ExecutePerspsDevToTensor, py::arg("surfaces"), py::arg("matrices_ptr"), py::arg("max_n"),
           py::arg("index_ptr"), py::arg("count_ptr"), py::arg("ptr"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr,
           py::arg("bgr") = false, py::arg("border") = std::array<int64_t, 3>{0, 0, 0}, py::arg("border_mode") = 0u, py::arg("row_stride") = 0,
           py::arg("plane_stride") = 0, py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::arg("matrix_stride") = 36u,
           py::arg("index_stride") = 4u, py::arg("max_step") = 0.0f, py::call_guard<py::gil_scoped_release>(),
           "ExecuteWarpsDevToTensor for perspective warps: job k = nine float32 (m00 m01 m02 m10 m11 m12 m20 m21 m22) at matrices_ptr + k matrix_stride, "
           "the inverse 3 x 3 homography; a pixel with w <= 0 takes the border in both modes.  The kernel reads matrices, indices and count when it runs on "
           "the task's stream: no sync, no copy to the host, capturable.  An invalid job (a coefficient that is not finite or above 2^24, a surface index "
           "outside the list) gives the normalised border; frames at or behind the count are not written.  max_step: the LDS hint (0 = none).  At most 128 "
           "surfaces; one dispatch")
      .def("ExecuteWarpsDevToTensor", &PySurfaceConvertResizer::ExecuteWarpsDevToTensor, py::arg("surfaces"), py::arg("matrices_ptr"), py::arg("max_n"),
           py::arg("index_ptr"), py::arg("count_ptr"), py::arg("ptr"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr,
           py::arg("bgr") = false, py::arg("border") = std::array<int64_t, 3>{0, 0, 0}, py::arg("border_mode") = 0u, py::arg("row_stride") = 0,
           py::arg("plane_stride") = 0, py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::arg("matrix_stride") = 24u,
           py::arg("index_stride") = 4u, py::arg("max_step") = 0.0f, py::call_guard<py::gil_scoped_release>(),
           "Up to max_n affine warps whose matrices lie in DEVICE memory: job k = six float32 (m00 m01 m02 m10 m11 m12) at matrices_ptr + k matrix_stride, "
           "its surface index one int32 at index_ptr + k index_stride (0 = every job samples surface 0), the first *count_ptr (a device int32; 0 = max_n) "
           "of them warped to the task's destination size and normalised into frame k of a planar tensor [max_n, 3, dh, dw] at device address ptr (strides "
           "in bytes, 0 = contiguous).  The kernel reads matrices, indices and count when it runs on the task's stream: no sync, no copy to the host, "
           "capturable.  An invalid job (a coefficient that is not finite or exceeds 2^24, no such surface) gives a frame of the normalised border; frames "
           "at or behind the count are not written.  max_step: the caller's bound on |m00| + |m01| and |m10| + |m11| that sizes the LDS (0 = none).  At "
           "most 128 surfaces; one dispatch")
      .def("ExecuteWarpsToTensor", &PySurfaceConvertResizer::ExecuteWarpsToTensor, py::arg("surfaces"), py::arg("surface_index"), py::arg("matrices"),
           py::arg("ptr"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr, py::arg("bgr") = false,
           py::arg("border") = std::array<int64_t, 3>{0, 0, 0}, py::arg("border_mode") = 0u, py::arg("row_stride") = 0, py::arg("plane_stride") = 0,
           py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::call_guard<py::gil_scoped_release>(),
           "K affine warps of the surfaces: job i samples surfaces[surface_index[i]] through the inverse 2 x 3 matrix matrices[i] (six floats) into the "
           "task's destination size, normalised, into a planar tensor [K, 3, dh, dw] at device address ptr (strides in bytes, 0 = contiguous); one "
           "dispatch per 96 regions")
      .def("ExecutePerspsToTensor", &PySurfaceConvertResizer::ExecutePerspsToTensor, py::arg("surfaces"), py::arg("surface_index"), py::arg("matrices"),
           py::arg("ptr"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr, py::arg("bgr") = false,
           py::arg("border") = std::array<int64_t, 3>{0, 0, 0}, py::arg("border_mode") = 0u, py::arg("row_stride") = 0, py::arg("plane_stride") = 0,
           py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::call_guard<py::gil_scoped_release>(),
           "K perspective warps of the surfaces: job i samples surfaces[surface_index[i]] through the inverse 3 x 3 matrix matrices[i] (nine floats, row-major: "
           "destination pixel -> homogeneous source coordinates) into the task's destination size, normalised, into a planar tensor [K, 3, dh, dw] at device "
           "address ptr (strides in bytes, 0 = contiguous); a pixel with w <= 0 takes the border in both modes; one dispatch per 82 regions")
      .def("ExecuteLetterboxToTensor", &PySurfaceConvertResizer::ExecuteLetterboxToTensor, py::arg("surfaces"), py::arg("rois"), py::arg("dst_rects"),
           py::arg("ptr"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr, py::arg("bgr") = false,
           py::arg("pad") = std::vector<int64_t>{0, 0, 0}, py::arg("row_stride") = 0, py::arg("plane_stride") = 0, py::arg("frame_stride") = 0,
           py::arg("channels_last") = false, py::call_guard<py::gil_scoped_release>(),
           "K letterbox jobs: rectangle rois[i] = (surface_index, x, y, w, h) resized into dst_rects[i] = (ix, iy, iw, ih) of its [3, dh, dw] frame of the "
           "planar tensor at device address ptr, pad (per output channel, 0..255) everywhere else in the frame, normalised (strides in bytes, 0 = "
           "contiguous); one dispatch per 82 regions.  ValueError for a bad pad and for rois / dst_rects of different lengths")
      .def("ExecuteLetterboxAAToTensor", &PySurfaceConvertResizer::ExecuteLetterboxAAToTensor, py::arg("surfaces"), py::arg("rois"), py::arg("dst_rects"),
           py::arg("ptr"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr, py::arg("bgr") = false,
           py::arg("pad") = std::vector<int64_t>{0, 0, 0}, py::arg("row_stride") = 0, py::arg("plane_stride") = 0, py::arg("frame_stride") = 0,
           py::arg("channels_last") = false, py::call_guard<py::gil_scoped_release>(),
           "ExecuteLetterboxToTensor with the antialiasing triangle filter (PIL's BILINEAR, torch's antialias=True) inside every dst_rect: every source "
           "pixel of a rectangle contributes, whatever the down-scale factor; the same arguments, refusals and ValueErrors")
      .def("ExecuteLetterboxDevToTensor", &PySurfaceConvertResizer::ExecuteLetterboxDevToTensor, py::arg("surfaces"), py::arg("boxes_ptr"), py::arg("max_n"),
           py::arg("count_ptr"), py::arg("rects_ptr"), py::arg("ptr"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr,
           py::arg("bgr") = false, py::arg("pad") = std::vector<int64_t>{0, 0, 0}, py::arg("row_stride") = 0, py::arg("plane_stride") = 0,
           py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::arg("box_stride") = 20u, py::arg("rect_stride") = 16u,
           py::call_guard<py::gil_scoped_release>(),
           "Up to max_n letterbox jobs whose boxes lie in DEVICE memory: entry k = five int32 (surface_index, x, y, w, h) at boxes_ptr + k box_stride, its "
           "placement four int32 (ix, iy, iw, ih) at rects_ptr + k rect_stride (0 = the kernel fits the box into the task's destination size, "
           "aspect-preserving and centred), the first *count_ptr (a device int32; 0 = max_n) of them resized into their placement of frame k of a planar "
           "tensor [max_n, 3, dh, dw] at device address ptr, pad (per output channel, 0..255) everywhere else in the frame, normalised (strides in bytes, "
           "0 = contiguous).  The kernel reads boxes, placements and count when it runs on the task's stream: no sync, no copy to the host, capturable.  "
           "An invalid box or placement gives a frame of the normalised pad; frames at or behind the count are not written.  At most 128 surfaces; one "
           "dispatch.  ValueError for a bad pad")
      .def("ExecuteRemapToTensor", &PySurfaceConvertResizer::ExecuteRemapToTensor, py::arg("surfaces"), py::arg("xmap_ptr"), py::arg("ymap_ptr"), py::arg("ptr"),
           py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr, py::arg("bgr") = false,
           py::arg("border") = std::array<int64_t, 3>{0, 0, 0}, py::arg("border_mode") = 0u, py::arg("row_stride") = 0, py::arg("plane_stride") = 0,
           py::arg("frame_stride") = 0, py::arg("channels_last") = false, py::arg("xmap_pitch") = 0u, py::arg("ymap_pitch") = 0u, py::arg("map_stride") = 0,
           py::arg("max_step") = 0.0f, py::call_guard<py::gil_scoped_release>(),
           "Per-pixel remap of the surfaces: frame i of a planar tensor [n, 3, dh, dw] at device address ptr (strides in bytes, 0 = contiguous) is "
           "surfaces[i] sampled at (xmap[y][x], ymap[y][x]) — float32 maps of the task's destination size in DEVICE memory at xmap_ptr / ymap_ptr + "
           "i map_stride (0 = every frame shares one pair), rows xmap_pitch / ymap_pitch bytes apart (0 = tight) — and normalised.  The kernel reads the "
           "maps when it runs on the task's stream: no sync, no copy to the host, capturable.  A NaN coordinate takes the border in both modes.  "
           "max_step: the caller's bound on the source pixels per destination pixel step of the maps, which sizes the LDS (0 = none); one dispatch per "
           "96 frames")
      .def("Stream", &PySurfaceConvertResizer::GetStream, "the hipStream_t every Execute* launches on (as an integer)")
      .def("DstSize", [](const PySurfaceConvertResizer& r) { return py::make_tuple(r.task_dst_w_, r.task_dst_h_); }, "(width, height) of the output");

  py::class_<PyTensorToSurface>(m, "PyTensorToSurface",
                                "Additive: a planar float tensor [N, 3, H, W] (dtype 0 f32, 1 f16, 2 bf16) -> NV12 / YUV420 in one pass: denormalise, "
                                "quantise (round to nearest even), BT.601 RGB -> YUV, 4:2:0; the bytes of PySurfaceConverter RGB_PLANAR -> YUV420 "
                                "(-> NV12) on the quantised planes.")
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format out, uint32_t gpu) { return new PyTensorToSurface(w, h, out, ctx_of((int)gpu), str_of((int)gpu)); }),
           py::arg("width"), py::arg("height"), py::arg("dst_format"), py::arg("gpu_id"))
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format out, size_t ctx, size_t str) { return new PyTensorToSurface(w, h, out, (HipContext)ctx, (HipStream)str); }),
           py::arg("width"), py::arg("height"), py::arg("dst_format"), py::arg("context"), py::arg("stream"))
      .def("Format", &PyTensorToSurface::GetFormat)
      .def("Execute", &PyTensorToSurface::Execute, py::arg("src"), py::arg("dtype"), py::arg("mean"), py::arg("std"), py::arg("cc_ctx") = nullptr,
           py::arg("bgr") = false, py::arg("row_pitch") = 0, py::arg("plane_stride") = 0, py::arg("channels_last") = false, py::keep_alive<0, 1>(),
           py::call_guard<py::gil_scoped_release>())
      .def("ExecuteBatch", &PyTensorToSurface::ExecuteBatch, py::arg("src"), py::arg("dst"), py::arg("dtype"), py::arg("mean"), py::arg("std"),
           py::arg("cc_ctx") = nullptr, py::arg("bgr") = false, py::arg("row_pitch") = 0, py::arg("plane_stride") = 0, py::arg("frame_stride") = 0,
           py::arg("channels_last") = false, py::call_guard<py::gil_scoped_release>())
      .def("Stream", &PyTensorToSurface::GetStream, "the hipStream_t every Execute* launches on (as an integer)")
      .def("Size", [](const PyTensorToSurface& t) { return py::make_tuple(t.Width(), t.Height()); }, "(width, height) of the frames")
      .def("Device", &PyTensorToSurface::Device, "the GPU the converter was built for; -1: whatever device is current (a foreign context handle)");

  py::class_<PySurfaceResizer>(m, "PySurfaceResizer")
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format f, uint32_t gpu) { return new PySurfaceResizer(w, h, f, ctx_of((int)gpu), str_of((int)gpu)); }),
           py::arg("width"), py::arg("height"), py::arg("format"), py::arg("gpu_id"))
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format f, size_t ctx, size_t str) { return new PySurfaceResizer(w, h, f, (HipContext)ctx, (HipStream)str); }),
           py::arg("width"), py::arg("height"), py::arg("format"), py::arg("context"), py::arg("stream"))
      .def("Format", &PySurfaceResizer::GetFormat)
      .def("SetInterpolation", &PySurfaceResizer::SetInterpolation, py::arg("interp"),
           "additive: 0 nearest, 1 bilinear, 2 Lanczos-3 (default: the filter the reference requests from NPP)")
      .def("GetInterpolation", &PySurfaceResizer::GetInterpolation)
      .def("SetAsync", &PySurfaceResizer::SetAsync, py::arg("on"),
           "additive: Execute() no longer waits for the stream (like PySurfaceConverter); default False = the reference's blocking behaviour")
      .def("GetAsync", &PySurfaceResizer::GetAsync)
      .def("Execute", &PySurfaceResizer::Execute, py::arg("src"), py::keep_alive<0, 1>(), py::call_guard<py::gil_scoped_release>())
      .def("ExecuteBatch", &PySurfaceResizer::ExecuteBatch, py::arg("src"), py::arg("dst"), py::call_guard<py::gil_scoped_release>(),
           "additive: n same-shape surfaces into n caller-owned surfaces, all planes of all frames in as few dispatches as possible; asynchronous on the resizer's stream");

  using FMap = py::array_t<float, py::array::c_style | py::array::forcecast>;
  py::class_<PySurfaceRemaper>(m, "PySurfaceRemaper")
      .def(py::init([](FMap& x, FMap& y, Pixel_Format f, uint32_t gpu) { return new PySurfaceRemaper(x, y, f, ctx_of((int)gpu), str_of((int)gpu)); }),
           py::arg("x_map"), py::arg("y_map"), py::arg("format"), py::arg("gpu_id"))
      .def(py::init([](FMap& x, FMap& y, Pixel_Format f, size_t ctx, size_t str) { return new PySurfaceRemaper(x, y, f, (HipContext)ctx, (HipStream)str); }),
           py::arg("x_map"), py::arg("y_map"), py::arg("format"), py::arg("context"), py::arg("stream"))
      .def("Format", &PySurfaceRemaper::GetFormat)
      .def("SetAsync", &PySurfaceRemaper::SetAsync, py::arg("on"), "additive: Execute() no longer waits for the stream; default False = the reference's blocking behaviour")
      .def("GetAsync", &PySurfaceRemaper::GetAsync)
      .def("Execute", &PySurfaceRemaper::Execute, py::arg("src"), py::keep_alive<0, 1>(), py::call_guard<py::gil_scoped_release>())
      .def("ExecuteBatch", &PySurfaceRemaper::ExecuteBatch, py::arg("src"), py::arg("dst"), py::call_guard<py::gil_scoped_release>(),
           "additive: the remaper's maps applied to n surfaces into n caller-owned surfaces, one dispatch per 32 frames; asynchronous on the remaper's stream");

  py::class_<PyFrameUploader>(m, "PyFrameUploader")
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format f, uint32_t gpu) { return new PyFrameUploader(w, h, f, ctx_of((int)gpu), str_of((int)gpu)); }),
           py::arg("width"), py::arg("height"), py::arg("format"), py::arg("gpu_id"))
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format f, size_t ctx, size_t str) { return new PyFrameUploader(w, h, f, (HipContext)ctx, (HipStream)str); }),
           py::arg("width"), py::arg("height"), py::arg("format"), py::arg("context"), py::arg("stream"))
      .def("Format", &PyFrameUploader::GetFormat)
      .def("SetAsync", &PyFrameUploader::SetAsync, py::arg("on"), py::arg("in_place") = false,
           "additive: True = UploadSingleFrame returns once the copy is queued (the surface is valid in stream order on the uploader's stream; a "
           "page-locked source frame must stay untouched until that stream is synchronised).  Default False = wait for the copy, like the reference. "
           "VPF_HIP_UPLOAD_ASYNC=1 makes True the default.  in_place=True: ordinary numpy frames that come back may be page-locked and read where they "
           "lie as well (the caller promises for them what it promises for AllocPinned() frames); default: they are copied out before the call returns")
      .def("GetAsync", &PyFrameUploader::GetAsync)
      .def("UploadSingleFrame", [](PyFrameUploader& self, py::array_t<uint8_t>& f) { if (self.Vouches()) vouch_for_frame(f, f.data(), (size_t)f.size(), self.Device()); return self.Upload(f.mutable_data(), (size_t)f.size()); },
           py::arg("frame").noconvert(true), py::keep_alive<0, 1>())
      .def("UploadSingleFrame", [](PyFrameUploader& self, py::array_t<float>& f) { if (self.Vouches()) vouch_for_frame(f, f.data(), (size_t)f.size() * sizeof(float), self.Device()); return self.Upload(f.mutable_data(), (size_t)f.size() * sizeof(float)); },
           py::arg("frame").noconvert(true), py::keep_alive<0, 1>())
      .def("UploadSingleFrame", [](PyFrameUploader& self, py::array_t<uint16_t>& f) { if (self.Vouches()) vouch_for_frame(f, f.data(), (size_t)f.size() * sizeof(uint16_t), self.Device()); return self.Upload(f.mutable_data(), (size_t)f.size() * sizeof(uint16_t)); },
           py::arg("frame").noconvert(true), py::keep_alive<0, 1>());

  py::class_<PySurfaceDownloader>(m, "PySurfaceDownloader")
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format f, uint32_t gpu) { return new PySurfaceDownloader(w, h, f, ctx_of((int)gpu), str_of((int)gpu)); }),
           py::arg("width"), py::arg("height"), py::arg("format"), py::arg("gpu_id"))
      .def(py::init([](uint32_t w, uint32_t h, Pixel_Format f, size_t ctx, size_t str) { return new PySurfaceDownloader(w, h, f, (HipContext)ctx, (HipStream)str); }),
           py::arg("width"), py::arg("height"), py::arg("format"), py::arg("context"), py::arg("stream"))
      .def("Format", &PySurfaceDownloader::GetFormat)
      .def("DownloadSingleSurface", &PySurfaceDownloader::Download<uint8_t>, py::arg("surface"), py::arg("frame").noconvert(true))
      .def("DownloadSingleSurface", &PySurfaceDownloader::Download<float>, py::arg("surface"), py::arg("frame").noconvert(true))
      .def("DownloadSingleSurface", &PySurfaceDownloader::Download<uint16_t>, py::arg("surface"), py::arg("frame").noconvert(true));

  py::class_<PyBufferUploader>(m, "PyBufferUploader")
      .def(py::init([](uint32_t e, uint32_t n, uint32_t gpu) { return new PyBufferUploader(e, n, ctx_of((int)gpu), str_of((int)gpu)); }),
           py::arg("elem_size"), py::arg("num_elems"), py::arg("gpu_id"))
      .def(py::init([](uint32_t e, uint32_t n, size_t ctx, size_t str) { return new PyBufferUploader(e, n, (HipContext)ctx, (HipStream)str); }),
           py::arg("elem_size"), py::arg("num_elems"), py::arg("context"), py::arg("stream"))
      .def("UploadSingleBuffer", &PyBufferUploader::Upload, py::arg("array"));

  py::class_<PyCudaBufferDownloader>(m, "PyCudaBufferDownloader")
      .def(py::init([](uint32_t e, uint32_t n, uint32_t gpu) { return new PyCudaBufferDownloader(e, n, ctx_of((int)gpu), str_of((int)gpu)); }),
           py::arg("elem_size"), py::arg("num_elems"), py::arg("gpu_id"))
      .def(py::init([](uint32_t e, uint32_t n, size_t ctx, size_t str) { return new PyCudaBufferDownloader(e, n, (HipContext)ctx, (HipStream)str); }),
           py::arg("elem_size"), py::arg("num_elems"), py::arg("context"), py::arg("stream"))
      .def("DownloadSingleCudaBuffer", &PyCudaBufferDownloader::Download, py::arg("buffer"), py::arg("array"));

#ifdef VPF_WITH_LIBAV
  py::class_<PyFfmpegDecoder>(m, "PyFfmpegDecoder")
      .def(py::init<const std::string&, const std::map<std::string, std::string>&, int>(), py::arg("input"), py::arg("opts"),
           py::arg("gpu_id") = 0)
      .def("Width", &PyFfmpegDecoder::Width)
      .def("Height", &PyFfmpegDecoder::Height)
      .def("Framerate", &PyFfmpegDecoder::Framerate)
      .def("ColorSpace", &PyFfmpegDecoder::GetColorSpace)
      .def("ColorRange", &PyFfmpegDecoder::GetColorRange)
      .def("Format", &PyFfmpegDecoder::GetPixelFormat)
      .def("DecodeSingleFrame", &PyFfmpegDecoder::DecodeSingleFrame, py::arg("frame"))
      .def("DecodeSingleSurface", &PyFfmpegDecoder::DecodeSingleSurface, py::keep_alive<0, 1>());
  m.attr("HAVE_LIBAV") = true;
#else
  m.attr("HAVE_LIBAV") = false;
#endif
  m.def("GetNumGpus", []() { return (int)HipResMgr::Instance().GetNumGpus(); });
  // --- additive helpers (not in the reference) ---
  m.def("GetContext", [](int gpu) { return (size_t)ctx_of(gpu); }, py::arg("gpu_id"), "opaque context cookie of a GPU ordinal");
  m.def("GetStream", [](int gpu) { return (size_t)str_of(gpu); }, py::arg("gpu_id"), "the per-GPU non-blocking hipStream_t used by the gpu_id overloads");
  m.def("SetExtendedColorspaces", &SetExtendedColorspaces, py::arg("on"),
        "also accept colour-space/range combinations the reference's converters reject although the kernels implement them");
  m.def("ConverterPairSupport", &ConvertSurface::PairSupport, py::arg("src_format"), py::arg("dst_format"),
        "1: pair exists in the reference's ConvertSurface, 2: additive pair, 0: unsupported");
  m.def("ConverterResolve",
        [](Pixel_Format in, Pixel_Format out, std::shared_ptr<ColorspaceConversionContext> cc) -> py::object {
          int cs = 0, cr = 0;
          if (!ConvertSurface::ResolveContext(in, out, cc.get(), &cs, &cr)) return py::none();
          return py::make_tuple(cs, cr);
        },
        py::arg("src_format"), py::arg("dst_format"), py::arg("cc_ctx") = nullptr,
        "(color_space, color_range) the converter would use for this pair and context, or None if it refuses the combination");
  m.def("LetterboxFit", [](uint32_t w, uint32_t h, uint32_t dw, uint32_t dh) {
          const vpf_rect r = vpf_letterbox_fit(vpf_size{w, h}, vpf_size{dw, dh});
          return py::make_tuple(r.x, r.y, r.width, r.height);
        }, py::arg("w"), py::arg("h"), py::arg("dw"), py::arg("dh"),
        "additive: (ix, iy, iw, ih), the aspect-preserving, centred placement of a w x h rectangle inside dw x dh (vpf_letterbox_fit; host only)");
  m.def("PerspMaxStep", [](const std::array<float, 9>& mat, uint32_t dw, uint32_t dh) { return vpf_persp_max_step(mat.data(), vpf_size{dw, dh}); },
        py::arg("matrix"), py::arg("dw"), py::arg("dh"),
        "additive: the LDS hint of ONE inverse 3 x 3 matrix (nine floats, row-major) for a dw x dh destination: the bound on the source pixels per "
        "destination pixel step, 0 where there is none (vpf_persp_max_step; host only)");
  m.def("KernelLibraryVersion", []() { return std::string(vpf_version()); });
  m.def("AllocPinned",
        [](size_t nbytes) {
          // numpy uint8 array over hipHostMalloc memory: PyFrameUploader DMAs from it directly (no staging memcpy)
          Buffer* b = Buffer::MakeOwnMem(nbytes, (HipContext)-1);
          py::capsule owner(b, [](void* p) { delete static_cast<Buffer*>(p); });
          return py::array_t<uint8_t>({(py::ssize_t)nbytes}, {(py::ssize_t)1}, b->GetDataAs<uint8_t>(), owner);
        },
        py::arg("nbytes"), "additive: page-locked host buffer as a numpy uint8 array (decode straight into it)");
  m.def("PinCacheStats", []() {
    const HostPinCache::Stats t = HostPinCache::stats();
    py::dict d;
    d["registered"] = t.registered; d["bytes"] = t.bytes; d["in_place"] = t.hits; d["staged"] = t.staged; d["evictions"] = t.evictions; d["failures"] = t.failures; d["budget"] = t.budget;
    return d;
  }, "additive: the cache of page-locked caller frame buffers (Tasks.hpp HostPinCache): buffers registered now, their bytes, uploads DMA'd in place / "
     "staged through a copy since start, registrations given up, registrations that failed");
  m.def("PinCacheDrop", []() { HostPinCache::drop_all(); }, "additive: unregister every page-locked caller buffer");
  m.def("PinCacheSetBudgetMB", [](size_t mb) { HostPinCache::set_budget_mb(mb); }, py::arg("mb"),
        "additive: switch the cache of page-locked caller frame buffers on (mb > 0: its byte budget) or off (0, the default unless VPF_HIP_PIN_CACHE_MB is set)");
  m.def("_UseHostAllocator", [](bool on) {
    static const DeviceAllocator host = {host_alloc, host_free, nullptr};
    SetDeviceAllocator(on ? &host : nullptr);
  }, py::arg("on"), "TEST HOOK: back Surfaces with host memory so geometry/dispatch can be unit-tested without a GPU");
}
