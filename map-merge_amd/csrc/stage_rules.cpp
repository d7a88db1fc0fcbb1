// stage_rules.cpp -- the policy of the opt-in stage selections (stage_rules.hpp): one row per stage, one line per conflict.
#include <string>

#include "stage_rules.hpp"

namespace mm3d {
namespace {

using Sel = const StageSelection &;

// In the order of `Stage`.  A new stage adds its row here -- and, if it cannot stand beside another, a line below.
const StageRule kRules[kStageCount] = {
    {"mm3d_set_icp_method", [](Sel s) { return s.icp != nullptr; },      // (no options: the method object is the selection)
     "point-to-plane ICP is selected", "shard bundles carry no normals for point-to-plane ICP"},
    {"mm3d_set_alignment", [](Sel s) { return s.align_options.method == MM3D_ALIGN_PREREJECTIVE; },
     "the prerejective alignment is selected", "the ranks' pair loops run SAC-IA, not the prerejective alignment"},
    {"mm3d_set_keypoints", [](Sel s) { return s.keypoint_options.source == MM3D_KEYPOINTS_UNIFORM; },
     "uniform keypoints are selected", nullptr},
    {"mm3d_set_refinement", [](Sel s) { return s.refine_options.method == MM3D_REFINE_NDT; },
     "NDT is selected", "shard bundles carry no voxel tables for NDT"},
    {"mm3d_set_coarse_alignment", [](Sel s) { return s.coarse_options.method == MM3D_COARSE_CORRELATIVE; },
     "the correlative alignment is selected", "shard bundles carry no signatures for the correlative alignment"},
    {"mm3d_set_confidence", [](Sel s) { return s.confidence_options.method == MM3D_CONFIDENCE_OVERLAP; },
     "the overlap confidence is selected", "shard bundles carry no tables for the overlap confidence"},
    {"mm3d_set_icp_rejection", [](Sel s) { return s.reject_options.one_to_one || s.reject_options.distance != MM3D_REJECT_NONE; },
     "a correspondence rejection is active", "the ranks' pair loops run the ICP without correspondence rejection"},
    {"mm3d_set_icp_geometry_rejection", [](Sel s) { return s.geometry_options.boundary || s.geometry_options.normals; },
     "a geometric rejector is active", "the ranks' pair loops run the ICP without the geometric rejectors"},
    {"mm3d_set_icp_robust", [](Sel s) { return s.robust_options.kernel != MM3D_ROBUST_OFF; },
     "a robust kernel is selected", "the ranks' pair loops run the ICP without a robust kernel"},
    {"mm3d_set_icp_color", [](Sel s) { return s.color_options.enabled != 0; },
     "coloured ICP is enabled", "shard bundles carry no colour gradients for coloured ICP"},
    {"mm3d_set_icp_generalized", [](Sel s) { return s.generalized_options.enabled != 0; },
     "generalized ICP is enabled", "shard bundles carry no normals for generalized ICP"},
    {"mm3d_set_estimator", [](Sel s) { return s.estimator_options.method == MM3D_ESTIMATOR_CONSISTENCY; },
     "the consistency estimation is selected", "the ranks' pair loops run RANSAC, not the consistency estimation"},
    {"mm3d_set_icp_sampling", [](Sel s) { return s.sampling_options.method != MM3D_ICP_SAMPLE_NONE; },
     "an ICP source sampling is set", "the ranks' pair loops run the ICP on the whole source, not on a sample"},
    {"mm3d_set_outlier_filter", [](Sel s) { return s.outlier_options.method == MM3D_OUTLIERS_STATISTICAL; },
     "the statistical outlier filter is selected", nullptr},
    {"mm3d_set_cluster_filter", [](Sel s) { return s.cluster_options.method != MM3D_CLUSTERS_OFF; },
     "the cluster filter is selected", nullptr},
    {"mm3d_set_smoothing", [](Sel s) { return s.smooth_options.method == MM3D_SMOOTH_MLS; },
     "the MLS smoothing is selected", nullptr},
    {"mm3d_set_planes", [](Sel s) { return s.plane_options.method != MM3D_PLANES_OFF; },
     "the plane stage is selected", nullptr},
};

// The unordered pairs that refuse each other, each once: whichever of the two is set second while the other is active is
// refused.  `only_while` narrows a pair to part of a stage's options.
struct Conflict { Stage a, b; bool (*only_while)(const StageSelection &); };
const Conflict kConflicts[] = {
    {Stage::Rejection, Stage::Color, nullptr},            // k_rej_reduce has no colour variant,
    {Stage::Rejection, Stage::Generalized, nullptr},      // nor a generalized one
    {Stage::Rejection, Stage::Robust, nullptr},           // the robust step weights every match: it has no correspondence stage
    {Stage::Geometry, Stage::Color, nullptr},             // step 1b is the rejecting step's
    {Stage::Geometry, Stage::Generalized, nullptr},
    {Stage::Geometry, Stage::Robust, nullptr},
    // a sample has no normals of its own index; the boundary rejector is target-side and composes with a sampler
    {Stage::Geometry, Stage::Sampling, [](Sel s) { return s.geometry_options.normals != 0; }},
    {Stage::Sampling, Stage::Refinement, nullptr},        // NDT searches nothing: there is no source sample for it to read
    {Stage::Sampling, Stage::Color, nullptr},             // the colour term reads the source's own records by index
    {Stage::Sampling, Stage::Generalized, nullptr},       // the source's normals are indexed by the source's own order
    {Stage::Color, Stage::Generalized, nullptr},          // one ICP stands in the default's place
    {Stage::Color, Stage::Robust, nullptr},               // k_rob_wave has point-to-point's and point-to-plane's terms only
    {Stage::Generalized, Stage::Robust, nullptr},
    {Stage::Robust, Stage::Refinement, nullptr},          // NDT has no correspondences to weight
};

}  // namespace

const StageRule &stage_rule(Stage st) { return kRules[(int)st]; }

bool StageSelection::rejecting() const { return stage_active(Stage::Rejection, *this); }
bool StageSelection::geometric() const { return stage_active(Stage::Geometry, *this); }
bool StageSelection::robust() const { return stage_active(Stage::Robust, *this); }

int refuse_device_list(mm3d_ctx *ctx, Stage st)
{
  ctx->err = std::string(stage_rule(st).setter) + ": not available on a device-list context";
  return MM3D_EUNSUPPORTED;
}

int select_stage(mm3d_ctx *ctx, Stage st, const std::function<void(StageSelection &)> &edit)
{
  const StageRule &rule = stage_rule(st);
  StageSelection next = ctx->sel;
  edit(next);
  if (rule.active(next)) {
    if (rule.stays_home && ctx->device_set) return refuse_device_list(ctx, st);
    for (const Conflict &c : kConflicts) {
      if (c.a != st && c.b != st) continue;
      const StageRule &other = stage_rule(c.a == st ? c.b : c.a);
      if (!other.active(next) || (c.only_while && !c.only_while(next))) continue;
      ctx->err = std::string(rule.setter) + ": not available while " + other.blocks + " (" + other.setter + ")";
      return MM3D_EUNSUPPORTED;
    }
  }
  auto commit = [&](mm3d_ctx *root) {
    edit(root->sel);
    for (mm3d_ctx *h : root->helpers) h->sel = root->sel;
  };
  commit(ctx);
  if (!rule.stays_home)
    for (mm3d_ctx *p : ctx->peers) commit(p);         // (every device of an mm3d_create_devices context)
  return MM3D_OK;
}

const StageRule *first_stage_left_home(const StageSelection &sel)
{
  for (const StageRule &r : kRules)
    if (r.stays_home && r.active(sel)) return &r;
  return nullptr;
}

}  // namespace mm3d
