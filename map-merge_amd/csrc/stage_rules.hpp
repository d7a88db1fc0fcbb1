// stage_rules.hpp -- which opt-in stage selections may stand together, which of them a device list and a shard carry, and what
// makes one active: one table (stage_rules.cpp), read by the seventeen setters through select_stage and by mm3d_shard_begin.
// Host code only; no kernel file's text is needed to read or to change the policy.
#pragma once

#include <functional>

#include "types.hpp"

#pragma GCC visibility push(hidden)
namespace mm3d {

enum class Stage {
  IcpMethod, Alignment, Keypoints, Refinement, Coarse, Confidence, Rejection, Geometry, Robust, Color, Generalized, Estimator,
  Sampling, Outliers, Clusters, Smoothing, Planes
};
constexpr int kStageCount = 17;

struct StageRule {
  const char *setter;                               // the call that selects the stage
  bool (*active)(const StageSelection &);           // the one place that says what "active" means for it (the options alone)
  const char *blocks;                               // what a setter that this stage blocks says of it
  const char *stays_home;                           // null: the stage's data travels in the device-list and shard bundles;
                                                    // else why it does not (mm3d_shard_begin's words)
};
const StageRule &stage_rule(Stage st);
inline bool stage_active(Stage st, const StageSelection &sel) { return stage_rule(st).active(sel); }

// The one way a context's stage selection changes (a setter, in its kernel file, under the context's lock and after its own
// validation).  `edit` is tried on a copy of the record first.  MM3D_EUNSUPPORTED, the context's error set and nothing changed,
// when `st` is active in the copy and either does not travel while the context is a device list or stands in a conflicting pair
// whose other side is active in the copy.  Else MM3D_OK: `edit` is applied to the context's record, which goes to every helper
// whole, and, when the stage travels, the same happens on every peer of a device list.
int select_stage(mm3d_ctx *ctx, Stage st, const std::function<void(StageSelection &)> &edit);
// "<setter>: not available on a device-list context" as the context's error; MM3D_EUNSUPPORTED
int refuse_device_list(mm3d_ctx *ctx, Stage st);
// the first active stage of `sel` that does not travel (its stays_home is what a shard says), or null
const StageRule *first_stage_left_home(const StageSelection &sel);

}  // namespace mm3d
#pragma GCC visibility pop
