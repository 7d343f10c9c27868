// csrc/typed_abi.h -- from an element type to the public entry points of that type: Abi<float>::head_forward is
// mms_head_forward_f32, Abi<double>::head_forward is mms_head_forward_f64.  Every entry point that another source of
// the library calls on its sequence route is here, one line each, so that a host template <typename T> calls
// Abi<T>::name(...) with the public argument list and no overload pair restates it.  AVE or MAX is chosen at the call
// site.  (csrc/layer_abi.hpp is the other library's table, of libmms_caffe.so's layers.)
#ifndef MMS_TYPED_ABI_H_
#define MMS_TYPED_ABI_H_

#include "mms_bn_maxpool.h"
#include "mms_conv_maxpool_stage.h"
#include "mms_conv_stage.h"
#include "mms_conv_stage_train.h"
#include "mms_head.h"

namespace mms {

template <typename T>
struct Abi;

template <>
struct Abi<float> {
  static constexpr auto conv_workspace_bytes = &mms_conv_workspace_bytes;
  static constexpr auto conv_forward = &mms_conv_forward_f32;
  static constexpr auto conv_backward = &mms_conv_backward_f32;
  static constexpr auto bn_pool_tanh_workspace_bytes = &mms_bn_pool_tanh_workspace_bytes;
  static constexpr auto bn_pool_tanh_forward = &mms_bn_pool_tanh_forward_f32;
  static constexpr auto bn_pool_tanh_backward = &mms_bn_pool_tanh_backward_f32;
  static constexpr auto bn_maxpool_tanh_forward = &mms_bn_maxpool_tanh_forward_f32;
  static constexpr auto bn_maxpool_tanh_backward = &mms_bn_maxpool_tanh_backward_f32;
  static constexpr auto conv_stage_workspace_bytes = &mms_conv_stage_workspace_bytes;
  static constexpr auto conv_stage_forward = &mms_conv_stage_forward_f32;
  static constexpr auto conv_maxpool_stage_workspace_bytes = &mms_conv_maxpool_stage_workspace_bytes;
  static constexpr auto conv_maxpool_stage_forward = &mms_conv_maxpool_stage_forward_f32;
  static constexpr auto conv_stage_train_workspace_bytes = &mms_conv_stage_train_workspace_bytes;
  static constexpr auto conv_stage_train_forward = &mms_conv_stage_train_forward_f32;
  static constexpr auto conv_stage_train_backward = &mms_conv_stage_train_backward_f32;
  static constexpr auto head_workspace_bytes = &mms_head_workspace_bytes;
  static constexpr auto head_forward = &mms_head_forward_f32;
  static constexpr auto head_backward = &mms_head_backward_f32;
};

template <>
struct Abi<double> {
  static constexpr auto conv_workspace_bytes = &mms_conv_workspace_bytes_f64;
  static constexpr auto conv_forward = &mms_conv_forward_f64;
  static constexpr auto conv_backward = &mms_conv_backward_f64;
  static constexpr auto bn_pool_tanh_workspace_bytes = &mms_bn_pool_tanh_workspace_bytes_f64;
  static constexpr auto bn_pool_tanh_forward = &mms_bn_pool_tanh_forward_f64;
  static constexpr auto bn_pool_tanh_backward = &mms_bn_pool_tanh_backward_f64;
  static constexpr auto bn_maxpool_tanh_forward = &mms_bn_maxpool_tanh_forward_f64;
  static constexpr auto bn_maxpool_tanh_backward = &mms_bn_maxpool_tanh_backward_f64;
  static constexpr auto conv_stage_workspace_bytes = &mms_conv_stage_workspace_bytes_f64;
  static constexpr auto conv_stage_forward = &mms_conv_stage_forward_f64;
  static constexpr auto conv_maxpool_stage_workspace_bytes = &mms_conv_maxpool_stage_workspace_bytes_f64;
  static constexpr auto conv_maxpool_stage_forward = &mms_conv_maxpool_stage_forward_f64;
  static constexpr auto conv_stage_train_workspace_bytes = &mms_conv_stage_train_workspace_bytes_f64;
  static constexpr auto conv_stage_train_forward = &mms_conv_stage_train_forward_f64;
  static constexpr auto conv_stage_train_backward = &mms_conv_stage_train_backward_f64;
  static constexpr auto head_workspace_bytes = &mms_head_workspace_bytes_f64;
  static constexpr auto head_forward = &mms_head_forward_f64;
  static constexpr auto head_backward = &mms_head_backward_f64;
};

}  // namespace mms
#endif  // MMS_TYPED_ABI_H_
