"""TEST-ONLY codec: PVQCodec's wire with the COMPUTE done by the CPU oracle (gq_oracle_pvq_encode + the HSQ level quantiser
and decode of tests/oracle_codec.py), so that the quantizers' host logic -- draw plan, wire offsets, error feedback,
two-phase -- runs for the ProbabilisticVectorCompressor on a machine without a GPU.  Never imported by the product."""
import numpy as np
import torch

import oracle
from gq_amd.codecs import PVQCodec
from gq_amd.compressors import ProbabilisticVectorCompressor
from oracle_codec import OracleHSQCodec, oracle_codec_factory, pack6


class OraclePVQCodec(PVQCodec):
    def encode_into(self, grad, wire_user, off, salt, r=None):
        c = self.c
        assert c._rng == "reference", "oracle codec: the reference's draws"
        want_levels = self._level_draws_wanted()
        if r is None:
            r_code = torch.rand(self.M)
            r_lvl = torch.rand(self.M) if want_levels else None
        else:
            r_code, r_lvl = r[:self.M], (r[self.M:2 * self.M] if want_levels else None)
        g = grad.detach().cpu().numpy().reshape(-1)
        codes_, u_ = oracle.pvq_encode(g, c.c_dagger.cpu().numpy(), r_code.cpu().numpy())
        codes, levels, lb_ub = self._views(wire_user, off)
        codes.copy_(torch.from_numpy(codes_.astype(np.uint8 if self.code_dtype == torch.uint8 else np.int32)))
        if not c.compressed_norm:
            levels.copy_(torch.from_numpy(u_))
            return
        lb, ub, lv = oracle.scalar_levels(u_, c.n_bit, 1 if want_levels else 0, r_lvl.cpu().numpy() if want_levels else None)
        if self.packed6:
            levels.copy_(torch.from_numpy(pack6(lv)))
        else:
            levels.copy_(torch.from_numpy(lv).to(self.level_dtype))
        lb_ub.copy_(torch.tensor([lb, ub], dtype=torch.float32))

    _decode = OracleHSQCodec._decode


def oracle_pvq_codec_factory(compressor, numel, shape, packed6=False):
    if isinstance(compressor, ProbabilisticVectorCompressor):
        return OraclePVQCodec(compressor, numel, shape, packed6)
    return oracle_codec_factory(compressor, numel, shape, packed6)
