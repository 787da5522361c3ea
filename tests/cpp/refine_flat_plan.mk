# builds the dump of plan_refine_flat (csrc/refine_flat_plan.h), host compiler only:  make -C tests/cpp -f refine_flat_plan.mk [OUT=path]
ROOT := ../..
CXX  ?= g++
CSRC := $(ROOT)/vector_line_quantization_amd/csrc
OUT  ?= refine_flat_plan_dump
all: $(OUT)
$(OUT): refine_flat_plan_dump.cpp $(CSRC)/refine_flat_plan.h $(CSRC)/flat_plan.h
	$(CXX) -std=c++17 -O1 -Wall -I$(CSRC) $< -o $@
clean:
	rm -f refine_flat_plan_dump
.PHONY: all clean
