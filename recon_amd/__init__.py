"""recon_amd — MI355X-native graph-context aggregation for RECON (GAT attention layer + GP-GNN
propagation), behind the reference's own nn.Module surface.  See DESIGN.md / INTEGRATION.md."""
__version__ = "0.1.0"

from .translation import translation_residuals  # noqa: E402,F401
from .char_features import char_word_features  # noqa: E402,F401
from .context_lstm import context_line_states  # noqa: E402,F401
from .sentence_lstm import pair_sentence_states  # noqa: E402,F401
from .transitions import pair_transitions  # noqa: E402,F401
from .pair_attention import pair_context_attention  # noqa: E402,F401
from .sentence_conv import sentence_conv_pool  # noqa: E402,F401
from .relation_head import relation_logits  # noqa: E402,F401
from .line_pool import entity_line_pool, entity_line_pool_ragged  # noqa: E402,F401
from .ragged_lines import RaggedLines  # noqa: E402,F401
from .pair_groups import PairGroups  # noqa: E402,F401
from .word_forms import WordForms, word_form_features  # noqa: E402,F401
from .objective import RelationMetrics, relation_objective  # noqa: E402,F401
from .context_batch import ContextBatcher, ContextTables, StageBBatch  # noqa: E402,F401
from .stage_b import EpochRows, StageBData, StageBSlice, run_epoch  # noqa: E402,F401
from .pair_data import PairData, PairSlice  # noqa: E402,F401
from .baselines import CNN, LSTM, PCNN, ContextAware  # noqa: E402,F401
