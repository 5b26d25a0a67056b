// tld_clip_keys.h -- whose entry of a CLIP state_dict a key is: one pure function of (tower, key) behind tld_clip_load_tensor and
// tld_clip_vis_load_tensor.  No HIP in here (tests/host/clip_keys_main.cpp compiles it alone).
//
// A full CLIP archive holds both towers and four scalars.  Each tower stores its own entries, passes over the other tower's and the scalars, and
// refuses the rest.  The text tower passes over anything under "visual." unread; the image tower knows the text side by name.
#pragma once

#include <string>

namespace tld {

enum ClipTower { CLIP_TEXT = 0, CLIP_IMAGE = 1 };
enum ClipKey { CLIP_KEY_MINE = 0, CLIP_KEY_OTHER = 1, CLIP_KEY_METADATA = 2, CLIP_KEY_UNKNOWN = 3 };

// the twelve entries of block l are under <prefix><l>.
inline const char* clip_block_prefix(ClipTower tower) { return tower == CLIP_TEXT ? "transformer.resblocks." : "visual.transformer.resblocks."; }

inline ClipKey route_clip_key(ClipTower tower, const std::string& k) {
    auto under = [&](const char* prefix) { return k.rfind(prefix, 0) == 0; };
    if (k == "logit_scale" || k == "input_resolution" || k == "context_length" || k == "vocab_size") return CLIP_KEY_METADATA;
    const bool text = k == "token_embedding.weight" || k == "positional_embedding" || k == "text_projection" || under("ln_final.") ||
                      under(clip_block_prefix(CLIP_TEXT));
    if (tower == CLIP_TEXT) return under("visual.") ? CLIP_KEY_OTHER : text ? CLIP_KEY_MINE : CLIP_KEY_UNKNOWN;
    const bool image = k == "visual.class_embedding" || k == "visual.positional_embedding" || k == "visual.proj" || k == "visual.conv1.weight" ||
                       under("visual.ln_pre.") || under("visual.ln_post.") || under(clip_block_prefix(CLIP_IMAGE));
    return image ? CLIP_KEY_MINE : text ? CLIP_KEY_OTHER : CLIP_KEY_UNKNOWN;
}

}  // namespace tld
