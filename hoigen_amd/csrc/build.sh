#!/bin/bash
# Build libhoigen_amd.so for gfx950 (cross-compiles without a GPU).
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 --offload-arch=gfx950 -fPIC -std=c++17 -Wall -Wno-unused-function -ffp-contract=fast ${HG_EXTRA_FLAGS}"   # HG_EXTRA_FLAGS=-DHG_STAMPS: diagnostic build with s_memtime stamps
OBJS=""
for f in hg_gemm hg_gemm_ring hg_gemm_ring2 hg_mlp_pair hg_mlp_pair256 hg_mlp_pair256p hg_gemm_duo hg_attn hg_attn_long hg_detr_attn hg_detr_rows hg_detr hg_detr_ffn hg_detr_dec hg_detr_ends hg_detr_heads hg_detr_neck hg_resnet_conv hg_resnet_stem hg_resnet_pool hg_resnet hg_qkv_attn hg_qkv_attn_text hg_text_grad hg_vae_fused hg_elem hg_adapter hg_adapter_long hg_preproc hg_preproc_batch hg_detector_views hg_hoi_head hg_region_props hg_detections hg_api hg_load hg_tower hg_text_bwd hg_heads hg_test_hooks; do
  # an object is rebuilt when its source, any header or include file here, or the C header is newer
  if [ ! -f $f.o ] || [ -n "$(find $f.hip *.h *.inc ../../include/hoigen_amd.h -newer $f.o)" ]; then
    rm -f $f.o
    # hg_preproc.hip is bit-exact arithmetic (Pillow's weight tables in double, torchvision's RoI-align in fp32, one rounding per
    # operation).  Under -ffp-contract=fast the backend fuses a multiply and an add whatever `#pragma clang fp contract(off)` says in
    # the source: roi_align_kernel got fma(b, scale, -0.5) and fma(ph, bh, sh), and one pooled value in six was an ulp or two off
    # torchvision's operation order (tests/test_gpu_roi_exact.py).  Nothing in that file gains from fused operations.
    # hg_hoi_head.hip takes its coordinates from roi_align_kernel's expressions and promises the same (tests/hoi_head_bound.py).
    X=""; [ $f = hg_preproc ] && X="-ffp-contract=off"
    [ $f = hg_hoi_head ] && X="-ffp-contract=off"
    # hg_region_props.hip: IoU, the prior row and the three linears are chains of separately rounded operations (tests/props_bound.py)
    [ $f = hg_region_props ] && X="-ffp-contract=off"
    # hg_detections.hip: box_iou and recover_boxes are chains of separately rounded operations - (x2 - x1) * (y2 - y1), cx - 0.5f * w and
    # (area_g + area_d) - inter fused would be an ulp off torchvision's order (tests/detections_bound.py)
    [ $f = hg_detections ] && X="-ffp-contract=off"
    # hg_preproc_batch.hip: the same weight tables as hg_preproc.hip, evaluated per crop on the device (hg_preproc_geom.h)
    [ $f = hg_preproc_batch ] && X="-ffp-contract=off"
    # hg_detector_views.hip: the same tables for whole images, and the size rule of the detector's resize in double (hg_detector_views_geom.h)
    [ $f = hg_detector_views ] && X="-ffp-contract=off"
    # hg_detr_neck.hip: the sine embedding's argument is a chain of separately rounded operations (tests/detr_neck_bound.py)
    [ $f = hg_detr_neck ] && X="-ffp-contract=off"
    ( $HIPCC $FLAGS $X -c $f.hip -o $f.o || rm -f $f.o ) &
  fi
  OBJS="$OBJS $f.o"
done
wait
for o in $OBJS; do [ -f $o ] || { echo "compile failed: $o"; exit 1; }; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined $OBJS -o libhoigen_amd.so
echo "built $(pwd)/libhoigen_amd.so"
