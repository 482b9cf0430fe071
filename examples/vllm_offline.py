"""The offline vLLM-style API on the HIP engine: several images, two samples each, vLLM 0.5.5 sampling parameters.

    python examples/vllm_offline.py /path/to/starvector-1b-im2svg image1.png [image2.png ...]
"""
import sys

from PIL import Image

from starvector_amd.vllm import LLM, SamplingParams

checkpoint, paths = sys.argv[1], sys.argv[2:]
llm = LLM(model=checkpoint, max_num_seqs=16, max_model_len=8192)
params = SamplingParams(n=2, temperature=0.6, top_p=0.9, min_p=0.02, frequency_penalty=0.1, max_tokens=4000, seed=0)
requests = [{"prompt": "<image-start>", "multi_modal_data": {"image": Image.open(p).convert("RGB")}} for p in paths]
for path, result in zip(paths, llm.generate(requests, params)):
    for sample in result.outputs:
        print(f"--- {path} sample {sample.index}: {len(sample.token_ids)} tokens, finish_reason={sample.finish_reason}")
        print(sample.text)
