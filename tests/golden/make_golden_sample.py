"""Sampled-decoding oracle: HF transformers itself, with a draw we can repeat.

    python tests/golden/make_golden_sample.py

Rebuilds the tiny LlamaForCausalLM of decode_tiny_llama.npz from that fixture's `p_*` arrays and calls HF
`generate(do_sample=True, ...)` with `torch.multinomial` replaced, for the duration of the call, by the inverse-CDF draw of
`_SampleState` (first index in vocabulary order whose inclusive cumulative probability exceeds u * total) fed by
`report_decoder.sample_uniform(seed, row, step)`.  Everything else -- processor order, warpers, min-length, EOS / pad handling,
stopping -- is HF's own code.  Stores the token streams, the seed and the argument sets in decode_tiny_llama_sample.npz.
(transformers 5.x applies no default top_k; older releases used 50.)  SEED was not changed after the first run: no draw of the four
sets lies on a cumulative-sum boundary (the CPU test compares the streams exactly)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from medical_image_analysis_amd.report_decoder import sample_uniform  # noqa: E402

SEED = 1234
CASES = {
    "plain": dict(max_new_tokens=12),
    "t07_k8": dict(max_new_tokens=12, temperature=0.7, top_k=8, min_new_tokens=2, repetition_penalty=2.0),
    "p09": dict(max_new_tokens=12, top_p=0.9, temperature=1.3, min_new_tokens=3),
    "k5p8": dict(max_new_tokens=12, top_k=5, top_p=0.8, repetition_penalty=1.5),
}


def main():
    from transformers import LlamaConfig, LlamaForCausalLM
    g = np.load(os.path.join(HERE, "decode_tiny_llama.npz"))
    cfg = LlamaConfig(vocab_size=48, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128, rms_norm_eps=1e-6, bos_token_id=1,
                      eos_token_id=2, pad_token_id=0, attention_bias=False, tie_word_embeddings=False)
    m = LlamaForCausalLM(cfg).eval()
    m.load_state_dict({k[2:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("p_")})
    emb, att = torch.from_numpy(g["inputs_embeds"]), torch.from_numpy(g["attention_mask"])
    real = torch.multinomial
    out, kept = {}, {}
    for name, kw in CASES.items():
        step, log = [0], []

        def draw(probs, num_samples=1, **_):
            c = probs.double().cumsum(-1)
            u = sample_uniform(SEED, probs.shape[0], step[0])
            step[0] += 1
            log.append((int((probs > 0).sum(-1).min()), int((probs > 0).sum(-1).max())))
            return (c <= u[:, None] * c[:, -1:]).sum(-1).clamp(max=probs.shape[1] - 1)[:, None]

        torch.multinomial = draw
        try:
            with torch.no_grad():
                o = m.generate(inputs_embeds=emb, attention_mask=att, do_sample=True, pad_token_id=0, eos_token_id=2, **kw)
        finally:
            torch.multinomial = real
        out["tokens_" + name] = o.numpy().copy()
        kept[name] = log
        print(name, o.tolist(), "kept (min, max) per step", log)
    np.savez(os.path.join(HERE, "decode_tiny_llama_sample.npz"), seed=np.int64(SEED), cases=np.array(json.dumps(CASES)), **out)


if __name__ == "__main__":
    main()
