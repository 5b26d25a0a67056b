// tld_param_layout.h -- THE flat fp32 parameter vector of the denoiser: Denoiser.named_parameters() order of the reference (tld/denoiser.py:85-114),
// i.e. the state_dict order without the two registered buffers (angular_speeds, precomputed_pos_enc).  The training engine binds its parameters,
// gradients, Adam moments and EMA copy in this order (tld_train_param_layout reports it; tests/test_train_host.py pins it), and the inference engine
// derives its weight images from a vector in it (tld_engine_refresh_weights).  Stated once, here.  Host-only, no HIP.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace tld {

struct ParamTensor { std::string key; int64_t off, numel; };

struct LayerOffsets {     // one decoder block; every block has the same size, so block i sits ParamLayout::layer_stride() * i behind block 0
    int64_t qkv, kv, q, up_w, up_b, dw_w, dw_b, down_w, down_b, n1w, n1b, n2w, n2b, n3w, n3b;
};

struct ParamLayout {
    std::vector<ParamTensor> tensors;
    int64_t count = 0;
    int64_t ff1w = 0, ff1b = 0, ff3w = 0, ff3b = 0, cvw = 0, cvb = 0, l1w = 0, l1b = 0, liw = 0, lib = 0, l2w = 0, l2b = 0, pos = 0, outw = 0, outb = 0, nw = 0,
            nb = 0, lbw = 0, lbb = 0;
    std::vector<LayerOffsets> layers;
    int64_t layer_stride() const { return layers.size() > 1 ? layers[1].qkv - layers[0].qkv : 0; }
};

// d = embed_dim, L = n_layers, ne = noise_embed_dims, pd = n_channels * patch_size^2, hid = mlp_multiplier * d, ntok = tokens per sample
inline ParamLayout make_param_layout(int d, int L, int ne, int pd, int hid, int ntok, int text) {
    ParamLayout p;
    auto add = [&p](const std::string& k, int64_t n, int64_t* off) {
        *off = p.count;
        p.tensors.push_back({k, p.count, n});
        p.count += n;
    };
    add("fourier_feats.1.weight", (int64_t)d * ne, &p.ff1w); add("fourier_feats.1.bias", d, &p.ff1b);
    add("fourier_feats.3.weight", (int64_t)d * d, &p.ff3w); add("fourier_feats.3.bias", d, &p.ff3b);
    const std::string blk = "denoiser_trans_block.";
    add(blk + "patchify_and_embed.0.weight", (int64_t)pd * pd, &p.cvw); add(blk + "patchify_and_embed.0.bias", pd, &p.cvb);
    add(blk + "patchify_and_embed.2.weight", pd, &p.l1w); add(blk + "patchify_and_embed.2.bias", pd, &p.l1b);
    add(blk + "patchify_and_embed.3.weight", (int64_t)d * pd, &p.liw); add(blk + "patchify_and_embed.3.bias", d, &p.lib);
    add(blk + "patchify_and_embed.4.weight", d, &p.l2w); add(blk + "patchify_and_embed.4.bias", d, &p.l2b);
    add(blk + "pos_embed.weight", (int64_t)ntok * d, &p.pos);
    p.layers.resize((size_t)L);
    for (int i = 0; i < L; ++i) {
        const std::string b = blk + "decoder_blocks." + std::to_string(i) + ".";
        LayerOffsets& q = p.layers[(size_t)i];
        add(b + "self_attention.qkv_linear.weight", (int64_t)3 * d * d, &q.qkv);
        add(b + "cross_attention.kv_linear.weight", (int64_t)2 * d * d, &q.kv);
        add(b + "cross_attention.q_linear.weight", (int64_t)d * d, &q.q);
        add(b + "mlp.mlp.0.weight", (int64_t)hid * d, &q.up_w); add(b + "mlp.mlp.0.bias", hid, &q.up_b);
        add(b + "mlp.mlp.1.weight", (int64_t)hid * 9, &q.dw_w); add(b + "mlp.mlp.1.bias", hid, &q.dw_b);
        add(b + "mlp.mlp.3.weight", (int64_t)d * hid, &q.down_w); add(b + "mlp.mlp.3.bias", d, &q.down_b);
        add(b + "norm1.weight", d, &q.n1w); add(b + "norm1.bias", d, &q.n1b);
        add(b + "norm2.weight", d, &q.n2w); add(b + "norm2.bias", d, &q.n2b);
        add(b + "norm3.weight", d, &q.n3w); add(b + "norm3.bias", d, &q.n3b);
    }
    add(blk + "out_proj.0.weight", (int64_t)pd * d, &p.outw); add(blk + "out_proj.0.bias", pd, &p.outb);
    add("norm.weight", d, &p.nw); add("norm.bias", d, &p.nb);
    add("label_proj.weight", (int64_t)d * text, &p.lbw); add("label_proj.bias", d, &p.lbb);
    return p;
}

}  // namespace tld
