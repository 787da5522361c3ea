# builds the dump of plan_sqflat_scan (csrc/sqflat_plan.h), host compiler only:  make -C tests/cpp -f sqflat_plan.mk [OUT=path]
ROOT := ../..
CXX  ?= g++
CSRC := $(ROOT)/vector_line_quantization_amd/csrc
OUT  ?= sqflat_plan_dump
all: $(OUT)
$(OUT): sqflat_plan_dump.cpp $(CSRC)/sqflat_plan.h $(CSRC)/sq_plan.h $(CSRC)/pq_plan.h $(CSRC)/scan_plan.h
	$(CXX) -std=c++17 -O1 -Wall -I$(CSRC) $< -o $@
clean:
	rm -f sqflat_plan_dump
.PHONY: all clean
